// nwc_sanitizer: concurrent one-message sanitize calls share one pipeline launch (include/nwc.h
// "sanitizer").  Included by nwc_api.hip after sanitizer.h and verifier.h.  The
// grouping itself is sanitize_queue.h (no HIP, tested on the CPU); this file is its device backend
// and the C entries; the layouts are msg_plan.h's (san_group_buf, san_scratch).
//
// A sanitizer owns SANITIZER_BUFFERS group buffers of coherent pinned host memory and one block of
// HBM scratch.  One group is one fixed sequence of launches on the device's stream -- k_parse_group,
// k_verify_msg_group, k_finalize_group (messages.h) -- enqueued under the device mutex, which is
// released before anyone polls; the host reads nothing back between the first launch and the result
// words the last kernel stores into the pinned buffer.  Groups follow each other in stream order,
// so the two buffers share the scratch.  A message larger than a group, and every message while the
// latency kernel's preconditions do not hold (the committee cache is the configured committee and
// has its combs; NWC_COLD and NWC_VERIFY_PATH at their defaults), is handed to
// nwc_sanitize_messages; so is a message whose result word asks for it (redo).
//
// Vote::new in the flight (nwc_sanitizer_sanitize_vote; vote.h): a request may carry a signer.  Its
// slot of the group buffer then holds the device address of the signer's key record, and a group
// with at least one such slot gets a fourth launch, k_vote_group, behind k_finalize_group: one wave
// per message, which signs where the slot has a key and the result word says Ok + header.  Groups
// without vote requests run the three launches above and nothing else.  A vote the flight did not
// deliver (the message was redone or bypassed, or the flag stayed unwritten) is signed by
// vote_alone: the header's author string and round cross the device's pinned stage and k_vote_wire
// decodes them as the parse does -- the host has no base64 decoder.
//
// Decoded views in the flight (nwc_sanitizer_sanitize_view): a request may ask for its
// message's nwc_msg_view.  A group with at least one such slot gets k_view_group behind
// k_finalize_group and before k_vote_group: one wave per message, which builds the record and the
// body of the slots that ask, from what the group's parse left in the scratch, into the slot's own
// region of the pinned buffer.  A view the flight did not deliver (the message was redone or
// bypassed, or the flag stayed unwritten) comes from view_alone: nwc_sanitize_messages_view on the
// one message, which for a redone or bypassed message is also its decision.
#include "sanitize_queue.h"

// one slack, spelled where each layer needs it: the kernel's region arithmetic, the queue's, the
// pinned layout's body area (byte_cap + slack x messages) and the bound the callers size a body by
static_assert(nwc::GROUP_VIEW_SLACK == nwc::sq::VIEW_SLACK && nwc::plan::SAN_VIEW_SLACK == nwc::sq::VIEW_SLACK,
              "the view body slack differs between messages.h, sanitize_queue.h and msg_plan.h");
static_assert(nwc::sq::VIEW_BYTES == nwc::plan::MSG_VIEW_BYTES && nwc::sq::VIEW_BYTES == 4 * nwc::VIEW_WORDS,
              "the view record's size differs between the layers");

namespace {

constexpr int SANITIZER_BUFFERS = 2;   // one group in flight, the next one filling

struct Sanitizer final : nwc::sq::Backend {
  std::atomic<DevCtx*> d{nullptr};   // nullptr once nwc_shutdown has taken the context
  uint32_t max_msgs = 0;
  uint64_t byte_cap = 0;
  nwc::plan::SanGroupBuf gl{};
  nwc::plan::SanScratch sl{};
  std::unique_ptr<Buf<uint8_t>> host[SANITIZER_BUFFERS];   // pinned; registered with the context's set under its mu
  std::unique_ptr<Buf<uint8_t>> scratch;                   // HBM, accounted under Scratch, kept by nwc_trim
  bool counters_dirty = false;   // an enqueue failed half way: zero the counters before the next group (under the context's mu)
  std::unique_ptr<nwc::sq::Queue> q;

  nwc::sq::GroupBuf view(uint8_t* p) const {
    nwc::sq::GroupBuf g;
    g.data = p + gl.data;
    g.starts = reinterpret_cast<uint64_t*>(p + gl.starts);
    g.lens = reinterpret_cast<uint32_t*>(p + gl.lens);
    g.gc_rounds = reinterpret_cast<uint64_t*>(p + gl.gc_rounds);
    g.targets = p + gl.targets;
    g.results = reinterpret_cast<uint32_t*>(p + gl.results);
    g.digests = p + gl.digests;
    g.kinds = p + gl.kinds;
    g.vote_keys = reinterpret_cast<uint64_t*>(p + gl.vote_keys);
    g.vote_sigs = p + gl.vote_sigs;
    g.vote_flags = p + gl.vote_flags;
    g.view_wanted = p + gl.view_wanted;
    g.views = p + gl.views;
    g.view_used = reinterpret_cast<uint32_t*>(p + gl.view_used);
    g.view_flags = p + gl.view_flags;
    g.view_body = p + gl.view_body;
    return g;
  }
  nwc::sq::GroupBuf buffer(int b) override { return view(host[b]->get()); }

  static bool groupable() {
    return g_cm_is_config.load() && g_cm_combs.load() && settings().cold && settings().verify_path == VPath::Default;
  }

  int launch(int b, uint32_t nmsg, uint64_t nbytes) override {
    DevCtx& dc = *d.load();
    std::lock_guard<std::mutex> lk(dc.mu);
    HIP_TRY(hipSetDevice(dc.hip_id));
    if (int rc = ensure_verify_tables(dc)) return rc;
    const nwc::sq::GroupBuf h = view(host[b]->get()), g = view(host[b]->dev());
    if (nmsg > max_msgs || nbytes > byte_cap) return set_err(NWC_ERR_ARG, "sanitizer: a group beyond its buffer");
    if (!groupable() || !dc.cc_stakes || !dc.cm_n || !dc.cm_comb || !dc.comb_base) {
      // the committee changed between the callers' check and this launch: every member takes the
      // batch entry with the committee of its own moment
      for (uint32_t i = 0; i < nmsg; ++i)
        __atomic_store_n(h.results + i, nwc::sq::R_WRITTEN | nwc::sq::R_REDO, __ATOMIC_RELEASE);
      return 0;
    }
    // what the members ask for, and everything that can fail without a launch, before anything is
    // queued: a group that fails frees its buffer at once, so no launch of it may be left behind
    bool views = false, votes = false;
    for (uint32_t i = 0; i < nmsg && !views; ++i) views = h.view_wanted[i] != 0;
    for (uint32_t i = 0; i < nmsg && !votes; ++i) votes = h.vote_keys[i] != 0;
    if (votes)
      if (int rc = ensure_sign_table(dc)) return rc;
    uint8_t* const base = scratch->get();
    uint32_t* const counters = arena_at<uint32_t>(base, sl.counters);
    const hipStream_t s = dc.stream;
    if (counters_dirty) {
      HIP_TRY(hipMemsetAsync(counters, 0, 8, s));
      counters_dirty = false;
    }
    counters_dirty = true;   // until the whole sequence is queued
    const uint64_t M = max_msgs;
    nwc::MsgArgs a{};
    a.data = g.data;   // read in place from the pinned buffer
    a.offsets = g.starts;   // (header_digest_one reads a message's start for its hashbuf slot)
    a.m = nmsg;
    a.hashbuf = arena_at<uint8_t>(base, sl.hashbuf);
    a.eq_msg = arena_at<uint8_t>(base, sl.eq_msg);
    a.cdig = a.eq_msg + 32 * M;
    a.eq_pk = arena_at<uint8_t>(base, sl.eq_pk);
    a.eq_sig = arena_at<uint8_t>(base, sl.eq_sig);
    a.v_pk = a.eq_pk + 32 * M;
    a.v_sig = a.eq_sig + 64 * M;
    uint32_t* const msg_index = arena_at<uint32_t>(base, sl.msg_index);
    a.v_msg = msg_index + M;
    a.v_total = counters;
    a.v_cap = sl.vote_slots;
    a.msg_base = (uint32_t)M;
    a.rec = arena_at<uint32_t>(base, sl.rec);
    a.rec_n = arena_at<uint32_t>(base, sl.rec_n);
    a.hmatch = arena_at<uint32_t>(base, sl.hmatch);
    a.digests = arena_at<uint8_t>(base, sl.digests);
    uint32_t* const list = arena_at<uint32_t>(base, sl.list);
    const nwc::Committee cm = committee_of(dc);
    const nwc::CommitteeCfg cc{dc.cc_stakes, dc.cc_worker_off, dc.cc_worker_ids, dc.cc_quorum, dc.cc_n};
    const size_t first_lds = 4 * (size_t)std::max<uint32_t>(1, std::min<uint32_t>(dc.cc_n, nwc::MSG_MAX_COMMITTEE));
    hipLaunchKernelGGL(nwc::k_parse_group, dim3(nmsg), dim3(64), first_lds, s, a, cm, cc,
                       nwc::GroupMsgs{g.starts, g.lens, g.gc_rounds, g.targets, list, counters + 1, (uint32_t)M, nmsg});
    HIP_TRY(hipGetLastError());
    // Header::digest (one SHA-512 chain per lane, ~0.2 ms whatever the group holds) in the first
    // blocks of the decide launch, beside the equations
    const uint32_t hd_blocks = (nmsg + 127) / 128;
    // at most one strict equation per message and one leaf per vote slot the group's bytes can hold
    const uint32_t eq_bound = nmsg + (uint32_t)nwc::plan::vote_slots(nbytes, 1);
    const nwc::VerifyArgs va{a.eq_msg, msg_index, 0, a.eq_pk, a.eq_sig, nullptr, sl.entries, 0, dc.base_table, dc.base24,
                             dc.scratch, dc.fb_list, dc.fb_count, 0u, cm};
    const nwc::CombArgs ca{nullptr, nullptr, dc.comb_base, dc.comb16, nullptr};
    hipLaunchKernelGGL(nwc::k_verify_msg_group, dim3(hd_blocks + eq_bound), dim3(128), 0, s, va, ca,
                       nwc::MsgGroupArgs{list, counters + 1, arena_at<uint8_t>(base, sl.modes), arena_at<uint8_t>(base, sl.vbytes),
                                         hd_blocks},
                       a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(nwc::k_finalize_group, dim3((nmsg + 255) / 256), dim3(256), 0, s, (const uint32_t*)a.rec,
                       (const uint32_t*)a.rec_n, (const uint32_t*)a.hmatch, (const uint8_t*)arena_at<uint8_t>(base, sl.vbytes),
                       (const uint8_t*)a.digests, (uint32_t)M, nmsg, nwc::GroupOut{g.results, g.digests, g.kinds},
                       knobs().sanitizer_redo_every.load(), counters, counters + 1);
    HIP_TRY(hipGetLastError());
    counters_dirty = false;
    // the views of the slots that ask, once their result words are out (stream order) and before the
    // votes: a view is a few loads and stores, a vote a signature
    if (views) {
      hipLaunchKernelGGL(nwc::k_view_group, dim3(nmsg), dim3(64), 0, s, a, cm,
                         nwc::GroupViews{g.view_wanted, reinterpret_cast<uint32_t*>(g.views), g.view_used, g.view_flags, g.view_body},
                         (const uint32_t*)g.results, (const uint64_t*)g.starts, (const uint32_t*)g.lens, nmsg);
      HIP_TRY(hipGetLastError());
    }
    // Vote::new for the slots that carry a key, once their result words are out (stream order)
    if (votes) {
      hipLaunchKernelGGL(nwc::k_vote_group, dim3(nmsg), dim3(64), 0, s, (const nwc::ge_niels*)dc.sign_table,
                         nwc::GroupVotes{g.vote_keys, g.vote_sigs, g.vote_flags}, (const uint32_t*)g.results,
                         (const uint32_t*)a.rec, (const uint8_t*)a.digests, (const uint8_t*)a.eq_pk, a.data,
                         (const uint64_t*)g.starts, (const uint32_t*)g.lens, nmsg);
      if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
        // the view launch is queued and writes into this buffer: it must have ended before the
        // group's members, who all leave with this error, give the buffer to the next group
        if (views) (void)hipStreamSynchronize(s);
        return set_err(NWC_ERR_DEVICE, "k_vote_group launch failed: %s", hipGetErrorString(e));
      }
    }
    return 0;
  }

  int wait(int /*b*/) override {
    DevCtx& dc = *d.load();
    std::lock_guard<std::mutex> lk(dc.mu);
    HIP_TRY(hipSetDevice(dc.hip_id));
    HIP_TRY(hipStreamSynchronize(dc.stream));
    return 0;
  }

  // the batch entry on this one message: the parent's route
  static int alone(const uint8_t* msg, size_t len, uint64_t gc_round, const uint8_t* vote_target, uint8_t* digest32, uint8_t* kind) {
    static const uint8_t none[16] = {0};
    const uint64_t offs[2] = {0, (uint64_t)len};
    int32_t code = 0;
    const int rc = nwc_sanitize_messages(len ? msg : none, offs, 1, gc_round, vote_target, &code, digest32, kind);
    return rc < 0 ? rc : (int)code;
  }
  int redo(const uint8_t* msg, size_t len, uint64_t gc_round, const uint8_t* vote_target, uint8_t* digest32, uint8_t* kind) override {
    return alone(msg, len, gc_round, vote_target, digest32, kind);
  }
  int bypass(const uint8_t* msg, size_t len, uint64_t gc_round, const uint8_t* vote_target, uint8_t* digest32,
             uint8_t* kind) override {
    return alone(msg, len, gc_round, vote_target, digest32, kind);
  }

  // the batch entry's view call on this one message: its decision and its view
  int view_alone(const uint8_t* msg, size_t len, uint64_t gc_round, const uint8_t* vote_target, uint8_t* digest32, uint8_t* kind,
                 const nwc::sq::ViewReq& out) override {
    static const uint8_t none[16] = {0};
    const uint64_t offs[2] = {0, (uint64_t)len};
    int32_t code = 0;
    const int rc = nwc_sanitize_messages_view(len ? msg : none, offs, 1, nullptr, gc_round, nullptr, vote_target, nullptr, &code,
                                              digest32, kind, nullptr, nullptr, out.rec, out.body, (size_t)out.body_cap,
                                              out.body_used);
    return rc < 0 ? rc : (int)code;
  }

  // Vote::new for one header the batch entry has accepted.  Only the bytes the vote needs cross
  // the stage: the variant, the author string and the round (the first 20 + L bytes, L the
  // string's length at byte 4).
  int vote_alone(const uint8_t* msg, size_t len, const uint8_t* id32, uint64_t vote_key, uint8_t* sig64) override {
    DevCtx* dp = d.load();
    if (!dp) return set_err(NWC_ERR_NOT_INIT, "the sanitizer's device context was shut down");
    DevCtx& dc = *dp;
    uint64_t L = 0;
    if (len >= 12) std::memcpy(&L, msg + 4, 8);
    if (len < 20 || L > len - 20) return set_err(NWC_ERR_ARG, "vote: the message holds no header author and round");
    const size_t need = 20 + (size_t)L, io = nwc::plan::align256(need + 16), so = io + 256, fo = so + 256;
    if (fo + 256 > NWC_PINNED_STAGE_MAX) return set_err(NWC_ERR_ARG, "vote: the author string does not fit the pinned stage");
    std::lock_guard<std::mutex> lk(dc.mu);
    HIP_TRY(hipSetDevice(dc.hip_id));
    if (int rc = ensure_sign_table(dc)) return rc;
    if (int rc = dc.ensure_pinned(NWC_PINNED_STAGE_MAX)) return rc;
    uint8_t* const hs = dc.pinned;
    uint8_t* const ds = dc.pinned.dev();
    std::memcpy(hs, msg, need);
    std::memset(hs + need, 0, io - need);
    std::memcpy(hs + io, id32, 32);
    std::memset(hs + so, 0, 64);
    hs[fo] = 0;
    hipLaunchKernelGGL(nwc::k_vote_wire, dim3(1), dim3(64), 0, dc.stream, reinterpret_cast<const nwc::SignKey*>(vote_key),
                       (const nwc::ge_niels*)dc.sign_table, (const uint8_t*)ds, (uint64_t)need, (const uint8_t*)(ds + io), ds + so,
                       ds + fo);
    HIP_TRY(hipGetLastError());
    if (!settings().spin_wait || !nwc::plan::poll_written(hs + fo, 1, std::chrono::milliseconds(200))) {
      HIP_TRY(hipStreamSynchronize(dc.stream));
      if (!nwc::plan::poll_written(hs + fo, 1, std::chrono::microseconds(0)))
        return set_err(NWC_ERR_DEVICE, "vote kernel left the signature unwritten");
    }
    std::memcpy(sig64, hs + so, 64);
    return 0;
  }

  // caller holds the context's mu (the handles leave its set)
  hipError_t release_buffers() {
    hipError_t first = hipSuccess;
    for (auto* p : {&host[0], &host[1], &scratch}) {
      if (!*p) continue;
      if (hipError_t e = (*p)->release(); first == hipSuccess) first = e;
      p->reset();
    }
    return first;
  }
};

std::mutex g_san_mu;   // guards g_sanitizers; taken after g_mu, never with a context's mu held
std::unordered_set<Sanitizer*> g_sanitizers;

// Stops a sanitizer's queue (queued requests finish, blocked callers are woken and leave) and frees
// its buffers once the streams have passed them.  Caller holds g_mu.
void sanitizer_retire(Sanitizer& v) {
  if (v.q) v.q->stop();
  DevCtx* dp = v.d.load();
  if (!dp) return;
  std::lock_guard<std::mutex> lk(dp->mu);
  (void)hipSetDevice(dp->hip_id);
  if (dp->stream) (void)hipStreamSynchronize(dp->stream);
  (void)v.release_buffers();
  v.d = nullptr;
}

// nwc_shutdown: live sanitizers finish what is queued and answer NWC_ERR_NOT_INIT from then on.
// Caller holds g_mu and no context's mu.
void sanitizers_shutdown() {
  std::lock_guard<std::mutex> vl(g_san_mu);
  for (Sanitizer* v : g_sanitizers) sanitizer_retire(*v);
}
}  // namespace

extern "C" {

void* nwc_sanitizer_create(uint32_t max_messages, uint32_t max_wait_us) {
  if (require_init()) return nullptr;
  // g_mu: the context cannot be shut down while the handle is built and registered
  std::lock_guard<std::mutex> gl(g_mu);
  DevCtx* dp = ctx(t_dev);
  if (!dp) { set_err(NWC_ERR_ARG, "device index %d not initialised", t_dev); return nullptr; }
  auto v = std::make_unique<Sanitizer>();
  v->d = dp;
  const uint32_t cap_msgs = settings().sanitizer_group_msgs;
  v->max_msgs = max_messages == 0 || max_messages > cap_msgs ? cap_msgs : max_messages;
  v->byte_cap = settings().sanitizer_group_bytes;
  v->gl = nwc::plan::san_group_buf(v->max_msgs, v->byte_cap);
  v->sl = nwc::plan::san_scratch(v->max_msgs, v->byte_cap);
  if (!v->sl.vote_slots || v->sl.entries > 0xFFFFFFFFull) { set_err(NWC_ERR_ARG, "sanitizer: group too large"); return nullptr; }
  {
    std::lock_guard<std::mutex> lk(dp->mu);
    if (!dp->cc_stakes) {
      set_err(NWC_ERR_NOT_INIT, "nwc_set_committee_config has not been called");
      return nullptr;
    }
    hipError_t e = hipSetDevice(dp->hip_id);
    for (int b = 0; e == hipSuccess && b < SANITIZER_BUFFERS; ++b) {
      v->host[b] = std::make_unique<Buf<uint8_t>>(dp->bufs, Account::Uncounted, Keep, nwc::buf::Kind::Pinned);
      e = v->host[b]->alloc(v->gl.bytes);
      if (e == hipSuccess) std::memset(v->host[b]->get(), 0, v->gl.bytes);
    }
    if (e == hipSuccess) {
      v->scratch = std::make_unique<Buf<uint8_t>>(dp->bufs, Account::Scratch, Keep);
      e = v->scratch->alloc(v->sl.bytes);
    }
    if (e == hipSuccess) {
      // everything zero (the counters among it); the constant parts of the equation space: a strict
      // equation checks its own message's digest under mode 1, a vote slot is a batch leaf (mode 0)
      uint8_t* const base = v->scratch->get();
      std::vector<uint32_t> own(v->max_msgs);
      for (uint32_t i = 0; i < v->max_msgs; ++i) own[i] = i;
      e = hipMemsetAsync(base, 0, v->sl.bytes, dp->stream);
      if (e == hipSuccess) e = hipMemsetAsync(base + v->sl.modes, 1, v->max_msgs, dp->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(base + v->sl.msg_index, own.data(), 4 * (size_t)v->max_msgs, hipMemcpyHostToDevice, dp->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(dp->stream);
    }
    if (e != hipSuccess) {
      (void)v->release_buffers();
      set_err(NWC_ERR_DEVICE, "sanitizer: group buffers (2 x %zu pinned bytes, %zu bytes of HBM) could not be set up: %s",
              v->gl.bytes, v->sl.bytes, hipGetErrorString(e));
      return nullptr;
    }
  }
  v->q = std::make_unique<nwc::sq::Queue>(*v, SANITIZER_BUFFERS, v->max_msgs, v->max_msgs, v->byte_cap, max_wait_us);
  std::lock_guard<std::mutex> vl(g_san_mu);
  g_sanitizers.insert(v.get());
  return v.release();
}

int nwc_sanitizer_sanitize(void* sanitizer, const uint8_t* msg, size_t len, uint64_t gc_round, const uint8_t* vote_target,
                           uint8_t digest32[32], uint8_t* kind) {
  if (!sanitizer) return set_err(NWC_ERR_ARG, "null sanitizer");
  if (len && !msg) return set_err(NWC_ERR_ARG, "null message");
  if (int rc = require_init()) return rc;
  Sanitizer& v = *static_cast<Sanitizer*>(sanitizer);
  t_code = 0;   // (a NWC_ERR_NOT_INIT of the batch entry keeps its own message)
  const int rc = v.q->submit(msg, len, gc_round, vote_target, digest32, kind, !Sanitizer::groupable());
  if (rc == NWC_ERR_NOT_INIT && t_code != NWC_ERR_NOT_INIT)
    return set_err(rc, "the sanitizer was destroyed or its device context shut down");
  return rc;
}

int nwc_sanitizer_sanitize_vote(void* sanitizer, void* signer, const uint8_t* msg, size_t len, uint64_t gc_round,
                                const uint8_t* vote_target, uint8_t digest32[32], uint8_t* kind, uint8_t vote_sig64[64],
                                int32_t* voted) {
  if (!sanitizer) return set_err(NWC_ERR_ARG, "null sanitizer");
  if (!vote_sig64 || !voted) return set_err(NWC_ERR_ARG, "null vote output");
  std::memset(vote_sig64, 0, 64);
  *voted = 0;
  if (len && !msg) return set_err(NWC_ERR_ARG, "null message");
  SIGNER_PROLOGUE(signer);
  Sanitizer& v = *static_cast<Sanitizer*>(sanitizer);
  DevCtx* const vd = v.d.load();
  if (!vd) return set_err(NWC_ERR_NOT_INIT, "the sanitizer was destroyed or its device context shut down");
  if (vd != sg.d) return set_err(NWC_ERR_ARG, "the signer lives on another device than the sanitizer");
  t_code = 0;
  const int rc = v.q->submit(msg, len, gc_round, vote_target, digest32, kind, !Sanitizer::groupable(),
                             (uint64_t)reinterpret_cast<uintptr_t>(sg.key), vote_sig64, voted);
  if (rc == NWC_ERR_NOT_INIT && t_code != NWC_ERR_NOT_INIT)
    return set_err(rc, "the sanitizer was destroyed or its device context shut down");
  return rc;
}

int nwc_sanitizer_sanitize_view(void* sanitizer, void* signer, const uint8_t* msg, size_t len, uint64_t gc_round,
                                const uint8_t* vote_target, uint8_t digest32[32], uint8_t* kind, uint8_t vote_sig64[64],
                                int32_t* voted, void* view, uint8_t* body, uint64_t body_cap, uint64_t* body_used) {
  if (!view)
    return signer ? nwc_sanitizer_sanitize_vote(sanitizer, signer, msg, len, gc_round, vote_target, digest32, kind, vote_sig64, voted)
                  : nwc_sanitizer_sanitize(sanitizer, msg, len, gc_round, vote_target, digest32, kind);
  // on an error < 0 the record is zero and no body byte is in use
  std::memset(view, 0, nwc::sq::VIEW_BYTES);
  if (body_used) *body_used = 0;
  if (signer && vote_sig64) std::memset(vote_sig64, 0, 64);
  if (signer && voted) *voted = 0;
  if (!sanitizer) return set_err(NWC_ERR_ARG, "null sanitizer");
  if (signer && (!vote_sig64 || !voted)) return set_err(NWC_ERR_ARG, "null vote output");
  if (len && !msg) return set_err(NWC_ERR_ARG, "null message");
  if (!body || !body_used) return set_err(NWC_ERR_ARG, "a view needs body and body_used");
  if (len >> 32) return set_err(NWC_ERR_ARG, "the message is 2^32 bytes or longer");
  if (body_cap < nwc::plan::view_body_bound(len, 1)) return set_err(NWC_ERR_ARG, "body_cap is below nwc_msg_view_body_bound(len, 1)");
  if (int rc = require_init()) return rc;
  Sanitizer& v = *static_cast<Sanitizer*>(sanitizer);
  uint64_t key = 0;
  if (signer) {
    Signer& sg = *static_cast<Signer*>(signer);
    if (!sg.d || !sg.key) return set_err(NWC_ERR_NOT_INIT, "the signer's device context was shut down");
    DevCtx* const vd = v.d.load();
    if (!vd) return set_err(NWC_ERR_NOT_INIT, "the sanitizer was destroyed or its device context shut down");
    if (vd != sg.d) return set_err(NWC_ERR_ARG, "the signer lives on another device than the sanitizer");
    key = (uint64_t)reinterpret_cast<uintptr_t>(sg.key);
  }
  const nwc::sq::ViewReq vr{static_cast<uint8_t*>(view), body, body_cap, body_used};
  t_code = 0;
  const int rc = v.q->submit(msg, len, gc_round, vote_target, digest32, kind, !Sanitizer::groupable(), key,
                             signer ? vote_sig64 : nullptr, signer ? voted : nullptr, &vr);
  if (rc == NWC_ERR_NOT_INIT && t_code != NWC_ERR_NOT_INIT)
    return set_err(rc, "the sanitizer was destroyed or its device context shut down");
  return rc;
}

int nwc_sanitizer_view_stats(void* sanitizer, uint64_t* in_flight, uint64_t* alone) {
  if (!sanitizer) return set_err(NWC_ERR_ARG, "null sanitizer");
  if (int rc = require_init()) return rc;
  const nwc::sq::Stats s = static_cast<Sanitizer*>(sanitizer)->q->stats();
  if (in_flight) *in_flight = s.views_in_flight;
  if (alone) *alone = s.views_alone;
  return 0;
}

int nwc_sanitizer_vote_stats(void* sanitizer, uint64_t* in_flight, uint64_t* alone) {
  if (!sanitizer) return set_err(NWC_ERR_ARG, "null sanitizer");
  if (int rc = require_init()) return rc;
  const nwc::sq::Stats s = static_cast<Sanitizer*>(sanitizer)->q->stats();
  if (in_flight) *in_flight = s.votes_in_flight;
  if (alone) *alone = s.votes_alone;
  return 0;
}

int nwc_sanitizer_stats(void* sanitizer, uint64_t* out) {
  if (!sanitizer || !out) return set_err(NWC_ERR_ARG, "null argument");
  const nwc::sq::Stats s = static_cast<Sanitizer*>(sanitizer)->q->stats();
  static_assert(sizeof(nwc_sanitizer_stats_t) == 8 * sizeof(uint64_t), "nwc_sanitizer_stats_t is eight counters");
  const nwc_sanitizer_stats_t t{s.groups, s.messages, s.bytes, s.equations, s.redone_messages, s.bypassed_messages,
                                s.max_messages_in_group, 0};
  std::memcpy(out, &t, sizeof t);
  return 0;
}

int nwc_sanitizer_destroy(void* sanitizer) {
  if (!sanitizer) return set_err(NWC_ERR_ARG, "null sanitizer");
  Sanitizer* v = static_cast<Sanitizer*>(sanitizer);
  {
    // g_mu: a concurrent nwc_shutdown either retires the sanitizer before this or finds it gone
    std::lock_guard<std::mutex> gl(g_mu);
    {
      std::lock_guard<std::mutex> vl(g_san_mu);
      g_sanitizers.erase(v);
    }
    sanitizer_retire(*v);
  }
  delete v;
  return 0;
}

}  // extern "C"
