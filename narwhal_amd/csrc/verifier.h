// nwc_verifier: concurrent small verify calls share one launch (include/nwc.h "verifier").
// Included by nwc_api.hip after the verification paths.  The grouping itself is verify_queue.h
// (no HIP, tested on the CPU); this file is its device backend and the C entries.
//
// A verifier owns VERIFIER_BUFFERS group buffers of coherent pinned host memory, read in place by
// k_verify_group_wide / k_verify_group_cold (kernels.hip) and written with one verdict byte per
// equation.  The leader of a group routes every equation on the host: a key found in the host view
// of the committee cache or of the auto key cache goes on the cached list (k_verify_group_wide, one
// launch per cache, on the device's own stream -- the caches are rebuilt in that stream's order),
// every other key on the first-sight list (k_verify_group_cold on the side stream: it reads only
// the basepoint comb, which lives until shutdown).  The device mutex is held to route and
// enqueue, never while anyone polls.
#include "verify_queue.h"

namespace {

constexpr int VERIFIER_BUFFERS = 2;   // one group in flight, the next one filling

struct Verifier final : nwc::vq::Backend {
  DevCtx* d = nullptr;   // nullptr once nwc_shutdown has taken the context
  int di = 0;
  uint32_t cap = 0, max_req = 0;
  bool grouping = true;  // false: every request is handed to the plain entries (no cold kernel in this process)
  uint8_t* host[VERIFIER_BUFFERS] = {};
  uint8_t* dev[VERIFIER_BUFFERS] = {};
  size_t o_mi = 0, o_pk = 0, o_sig = 0, o_mode = 0, o_list = 0, o_vb = 0, bytes = 0;
  std::vector<uint32_t> route_ak;       // launch(): the auto cache's equations (one launch at a time per buffer,
  std::mutex route_mu;                  // but two buffers may launch at once)
  std::mutex pend_mu;
  std::vector<uint8_t> pend_keys;       // first-sight keys of launched groups, for auto_insert (settle)
  std::unique_ptr<nwc::vq::Queue> q;

  void layout() {
    size_t o = align256(32 * (size_t)max_req);
    o_mi = o;   o += align256(4 * (size_t)cap);
    o_pk = o;   o += align256(32 * (size_t)cap);
    o_sig = o;  o += align256(64 * (size_t)cap);
    o_mode = o; o += align256(cap);
    o_list = o; o += align256(8 * (size_t)cap);
    o_vb = o;   o += align256(cap);
    bytes = o;
  }
  nwc::vq::GroupBuf view(uint8_t* p) const {
    nwc::vq::GroupBuf g;
    g.digests = p;
    g.msg_index = reinterpret_cast<uint32_t*>(p + o_mi);
    g.pks = p + o_pk;
    g.sigs = p + o_sig;
    g.modes = p + o_mode;
    g.lists = reinterpret_cast<uint32_t*>(p + o_list);
    g.vbytes = p + o_vb;
    return g;
  }
  nwc::vq::GroupBuf buffer(int b) override { return view(host[b]); }

  int launch(int b, uint32_t /*nreq*/, uint32_t neq, uint32_t& wide, uint32_t& cold) override {
    DevCtx& dc = *d;
    std::lock_guard<std::mutex> lk(dc.mu);
    HIP_TRY(hipSetDevice(dc.hip_id));
    const bool fresh = !dc.tables_ready;
    if (int rc = ensure_verify_tables(dc)) return rc;
    if (!dc.comb16) return set_err(NWC_ERR_DEVICE, "verifier: the basepoint comb is missing");
    const nwc::vq::GroupBuf h = view(host[b]), g = view(dev[b]);
    // route: committee equations from the front of the cached list, the auto cache's after them,
    // first-sight equations on the second list
    uint32_t ncm = 0, nak = 0, ncold = 0;
    uint32_t* cached = h.lists;
    uint32_t* first = h.lists + cap;
    {
      std::lock_guard<std::mutex> rl(route_mu);
      route_ak.clear();
      const bool cm_on = dc.cm_n && dc.cm_comb, ak_on = dc.ak_n && dc.ak_comb;
      std::unique_lock<std::mutex> hl(g_hcm.mu, std::defer_lock);
      if (cm_on) hl.lock();
      for (uint32_t e = 0; e < neq; ++e) {
        const uint8_t* pk = h.pks + 32 * (size_t)e;
        if (cm_on && g_hcm.idx.find(pk)) cached[ncm++] = e;
        else if (ak_on && dc.ak_host.find(pk)) route_ak.push_back(e);
        else first[ncold++] = e;
      }
      nak = (uint32_t)route_ak.size();
      if (nak) std::memcpy(cached + ncm, route_ak.data(), 4 * (size_t)nak);
    }
    wide = ncm + nak;
    cold = ncold;
    nwc::VerifyArgs a{g.digests, g.msg_index, 0, g.pks, g.sigs, nullptr, neq, 0, dc.base_table, dc.base24,
                      dc.scratch, dc.fb_list, dc.fb_count, 0u, nwc::Committee{}};
    const nwc::CombArgs ca{nullptr, nullptr, dc.comb_base, dc.comb16, nullptr};
    if (ncm) {
      a.committee = committee_of(dc);
      hipLaunchKernelGGL(nwc::k_verify_group_wide, dim3(ncm), dim3(128), 0, dc.stream, a, ca,
                         nwc::GroupArgs{g.lists, g.modes, g.vbytes, ncm});
      HIP_TRY(hipGetLastError());
    }
    if (nak) {
      ++dc.ak_hits;
      a.committee = auto_committee_of(dc);
      hipLaunchKernelGGL(nwc::k_verify_group_wide, dim3(nak), dim3(128), 0, dc.stream, a, ca,
                         nwc::GroupArgs{g.lists + ncm, g.modes, g.vbytes, nak});
      HIP_TRY(hipGetLastError());
    }
    if (ncold) {
      if (fresh) {
        // the tables were built on the device's stream by this very call
        HIP_TRY(hipEventRecord(dc.ev_fork, dc.stream));
        HIP_TRY(hipStreamWaitEvent(dc.side, dc.ev_fork, 0));
      }
      a.committee = nwc::Committee{};
      a.force_fb_every = settings().force_fallback_every;
      hipLaunchKernelGGL(nwc::k_verify_group_cold, dim3(ncold), dim3(256), 0, dc.side, a,
                         (const nwc::ge_niels_pad*)dc.comb16, nwc::GroupArgs{g.lists + cap, g.modes, g.vbytes, ncold});
      HIP_TRY(hipGetLastError());
      std::lock_guard<std::mutex> pl(pend_mu);
      for (uint32_t j = 0; j < ncold; ++j) {
        const uint8_t* pk = h.pks + 32 * (size_t)first[j];
        pend_keys.insert(pend_keys.end(), pk, pk + 32);
      }
    }
    return 0;
  }

  int wait(int /*b*/) override {
    DevCtx& dc = *d;
    std::lock_guard<std::mutex> lk(dc.mu);
    HIP_TRY(hipSetDevice(dc.hip_id));
    HIP_TRY(hipStreamSynchronize(dc.stream));
    HIP_TRY(hipStreamSynchronize(dc.side));
    return 0;
  }

  // launch_verify's general path (staged inputs, fallback and torsion passes) over the listed
  // equations, as verify_range's own second attempt
  int redo(int b, const uint32_t* idx, uint32_t m, bool strict, uint8_t* out) override {
    DevCtx& dc = *d;
    const nwc::vq::GroupBuf h = view(host[b]);
    std::lock_guard<std::mutex> lk(dc.mu);
    HIP_TRY(hipSetDevice(dc.hip_id));
    const uint64_t words = ((uint64_t)m + 63) / 64;
    const size_t need = align256(32 * (size_t)m) + align256(32 * (size_t)m) + align256(64 * (size_t)m) + align256(8 * (words + 1));
    if (int rc = dc.ensure_arena(need)) return rc;
    if (int rc = dc.ensure_pinned(NWC_PINNED_STAGE_MAX)) return rc;
    Carve c(dc.arena);
    uint8_t* dm = c.take<uint8_t>(32 * (size_t)m);
    uint8_t* dp = c.take<uint8_t>(32 * (size_t)m);
    uint8_t* ds = c.take<uint8_t>(64 * (size_t)m);
    uint64_t* dout = c.take<uint64_t>(8 * (words + 1));
    uint8_t* s = dc.pinned;
    for (uint32_t j = 0; j < m; ++j) {
      const uint32_t e = idx[j];
      std::memcpy(s + (dm - dc.arena) + 32 * (size_t)j, h.digests + 32 * (size_t)h.msg_index[e], 32);
      std::memcpy(s + (dp - dc.arena) + 32 * (size_t)j, h.pks + 32 * (size_t)e, 32);
      std::memcpy(s + (ds - dc.arena) + 64 * (size_t)j, h.sigs + 64 * (size_t)e, 64);
    }
    const size_t out_off = (size_t)((uint8_t*)dout - dc.arena);
    std::memset(s + out_off, 0, 8 * (words + 1));
    HIP_TRY(hipMemcpyAsync(dc.arena, s, out_off + 8 * (words + 1), hipMemcpyHostToDevice, dc.stream));
    if (int rc = launch_verify(dc, {.msgs = dm, .msg_stride = 1, .pks = dp, .sigs = ds, .n = m, .strict = strict ? 1 : 0,
                                    .out_words = dout, .stream = dc.stream, .flags = LV_OUT_ZEROED}))
      return rc;
    HIP_TRY(hipMemcpyAsync(s, dout, 8 * words, hipMemcpyDeviceToHost, dc.stream));
    HIP_TRY(hipStreamSynchronize(dc.stream));
    const uint64_t* w = reinterpret_cast<const uint64_t*>(s);
    for (uint32_t j = 0; j < m; ++j) out[j] = (uint8_t)((w[j >> 6] >> (j & 63)) & 1);
    return 0;
  }

  int bypass(const uint8_t* msg32, const uint8_t* pks, const uint8_t* sigs, size_t n, bool strict, uint8_t* valid) override {
    if (strict) {
      for (size_t i = 0; i < n; ++i) {
        const int rc = nwc_verify_strict(msg32, pks + 32 * i, sigs + 64 * i);
        if (rc < 0) return rc;
        valid[i] = rc == NWC_OK;
      }
      return 0;
    }
    std::vector<uint8_t> bad((n + 7) / 8, 0);
    const int rc = nwc_verify_batch(msg32, pks, sigs, n, bad.data());
    if (rc < 0) return rc;
    for (size_t i = 0; i < n; ++i) valid[i] = !((bad[i >> 3] >> (i & 7)) & 1);
    return 0;
  }

  // the first-sight keys of the groups launched so far join the auto cache as a small call's do
  // (the second sighting builds a key's tables), after the leader has its own answers
  void settle() override {
    std::vector<uint8_t> keys;
    {
      std::lock_guard<std::mutex> pl(pend_mu);
      keys.swap(pend_keys);
    }
    if (keys.empty()) return;
    DevCtx& dc = *d;
    std::lock_guard<std::mutex> lk(dc.mu);
    if (hipSetDevice(dc.hip_id) != hipSuccess) return;
    (void)auto_insert(dc, keys.data(), keys.size() / 32);   // an error here reaches the next call on the stream
  }

  void release_buffers() {
    for (int b = 0; b < VERIFIER_BUFFERS; ++b) {
      if (host[b]) (void)hipHostFree(host[b]);
      host[b] = dev[b] = nullptr;
    }
  }
};

std::mutex g_ver_mu;   // guards g_verifiers; taken after g_mu, never with a context's mu held
std::unordered_set<Verifier*> g_verifiers;

// Stops a verifier's queue (queued requests finish, blocked callers are woken and leave) and frees
// its buffers once the streams have passed them.  Caller holds g_mu.
void verifier_retire(Verifier& v) {
  if (v.q) v.q->stop();
  if (!v.d) return;
  DevCtx& dc = *v.d;
  std::lock_guard<std::mutex> lk(dc.mu);
  (void)hipSetDevice(dc.hip_id);
  if (dc.stream) (void)hipStreamSynchronize(dc.stream);
  if (dc.side) (void)hipStreamSynchronize(dc.side);
  v.release_buffers();
  v.d = nullptr;
}

// nwc_shutdown: live verifiers finish what is queued and answer NWC_ERR_NOT_INIT from then on.
// Caller holds g_mu and no context's mu.
void verifiers_shutdown() {
  std::lock_guard<std::mutex> vl(g_ver_mu);
  for (Verifier* v : g_verifiers) verifier_retire(*v);
}

int verifier_request(void* verifier, const uint8_t* msg32, const uint8_t* pks, const uint8_t* sigs, size_t n, bool strict,
                     uint8_t* valid) {
  Verifier& v = *static_cast<Verifier*>(verifier);
  if (!v.grouping) {
    if (!v.d) return set_err(NWC_ERR_NOT_INIT, "the verifier's device context was shut down");
    return v.bypass(msg32, pks, sigs, n, strict, valid);
  }
  const int rc = v.q->submit(msg32, pks, sigs, n, strict, valid);
  if (rc == NWC_ERR_NOT_INIT) return set_err(rc, "the verifier was destroyed or its device context shut down");
  return rc;
}

}  // namespace

extern "C" {

void* nwc_verifier_create(uint32_t max_requests, uint32_t max_wait_us) {
  if (require_init()) return nullptr;
  const int di = t_dev;
  DevCtx* dp = ctx(di);
  if (!dp) { set_err(NWC_ERR_ARG, "device index %d not initialised", di); return nullptr; }
  auto v = std::make_unique<Verifier>();
  v->d = dp;
  v->di = di;
  v->cap = settings().verifier_group_eq;
  v->max_req = max_requests == 0 || max_requests > v->cap ? v->cap : max_requests;
  // the first-sight kernel needs the basepoint comb, and the A/B paths (NWC_VERIFY_PATH, NWC_COLD=0)
  // are the plain entries' business
  v->grouping = settings().cold && settings().verify_path == VPath::Default;
  v->layout();
  if (v->grouping) {
    std::lock_guard<std::mutex> lk(dp->mu);
    bool ok = hipSetDevice(dp->hip_id) == hipSuccess;
    for (int b = 0; ok && b < VERIFIER_BUFFERS; ++b) {
      // coherent: the kernels' verdict bytes reach the host while it polls them
      void* p = nullptr;
      void* q = nullptr;
      ok = hipHostMalloc(&p, v->bytes, hipHostMallocCoherent) == hipSuccess;
      if (ok) v->host[b] = static_cast<uint8_t*>(p);
      ok = ok && hipHostGetDevicePointer(&q, p, 0) == hipSuccess;
      if (ok) v->dev[b] = static_cast<uint8_t*>(q);
    }
    if (!ok) {
      v->release_buffers();
      set_err(NWC_ERR_DEVICE, "verifier: pinned group buffers (%zu bytes each) could not be allocated", v->bytes);
      return nullptr;
    }
  }
  v->q = std::make_unique<nwc::vq::Queue>(*v, VERIFIER_BUFFERS, v->max_req, v->cap, std::min<uint32_t>(v->cap, NWC_WIDE_MAX),
                                          max_wait_us);
  std::lock_guard<std::mutex> vl(g_ver_mu);
  g_verifiers.insert(v.get());
  return v.release();
}

int nwc_verifier_verify_strict(void* verifier, const uint8_t msg32[32], const uint8_t pk[32], const uint8_t sig[64]) {
  if (!verifier || !msg32 || !pk || !sig) return set_err(NWC_ERR_ARG, "null argument");
  if (int rc = require_init()) return rc;
  uint8_t ok = 0;
  const int rc = verifier_request(verifier, msg32, pk, sig, 1, true, &ok);
  if (rc < 0) return rc;
  return ok ? NWC_OK : NWC_INVALID;
}

int nwc_verifier_verify_batch(void* verifier, const uint8_t msg32[32], const uint8_t* pks, const uint8_t* sigs, size_t n,
                              uint8_t* bad_bitmap) {
  if (!verifier) return set_err(NWC_ERR_ARG, "null verifier");
  if (n && (!msg32 || !pks || !sigs)) return set_err(NWC_ERR_ARG, "null buffer");
  if (int rc = require_init()) return rc;
  if (n == 0) return NWC_OK;   // empty iterator: dalek verify_batch of nothing is Ok
  std::vector<uint8_t> valid(n, 0);
  const int rc = verifier_request(verifier, msg32, pks, sigs, n, false, valid.data());
  if (rc < 0) return rc;
  bool all = true;
  for (size_t i = 0; i < n; ++i) all = all && valid[i];
  if (bad_bitmap) {
    std::memset(bad_bitmap, 0, (n + 7) / 8);
    for (size_t i = 0; i < n; ++i)
      if (!valid[i]) bad_bitmap[i >> 3] |= (uint8_t)(1u << (i & 7));
  }
  return all ? NWC_OK : NWC_INVALID;
}

int nwc_verifier_stats(void* verifier, uint64_t* out) {
  if (!verifier || !out) return set_err(NWC_ERR_ARG, "null argument");
  const nwc::vq::Stats s = static_cast<Verifier*>(verifier)->q->stats();
  static_assert(sizeof(nwc_verifier_stats_t) == 8 * sizeof(uint64_t), "nwc_verifier_stats_t is eight counters");
  const nwc_verifier_stats_t t{s.groups, s.requests, s.equations, s.wide_equations, s.cold_equations, s.redone_equations,
                               s.bypassed_requests, s.max_requests_in_group};
  std::memcpy(out, &t, sizeof t);
  return 0;
}

int nwc_verifier_destroy(void* verifier) {
  if (!verifier) return set_err(NWC_ERR_ARG, "null verifier");
  Verifier* v = static_cast<Verifier*>(verifier);
  {
    // g_mu: a concurrent nwc_shutdown either retires the verifier before this or finds it gone
    std::lock_guard<std::mutex> gl(g_mu);
    {
      std::lock_guard<std::mutex> vl(g_ver_mu);
      g_verifiers.erase(v);
    }
    verifier_retire(*v);
  }
  delete v;
  return 0;
}

}  // extern "C"
