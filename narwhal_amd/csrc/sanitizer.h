// Host side of the message pipeline (include/nwc.h nwc_sanitize_messages, nwc_dev_sanitize_messages
// and their _ex twins with per-message Core state and Vote::new; kernels in messages.h and vote.h;
// DESIGN §4.7, §4.13).  Included by nwc_api.hip after the device contexts and signer.h: uses
// DevCtx, set_err, HIP_TRY, launch_verify, the deferred-list helpers, Signer and
// ensure_sign_table.  Where a batch is cut, how its arenas are laid out and what a call defers are
// msg_plan.h's decisions; this file enqueues.
#pragma once

namespace {

using nwc::plan::MsgSchedule;

template <class T>
T* arena_at(uint8_t* base, size_t off) { return reinterpret_cast<T*>(base + off); }

// The copier thread of a staged host call: it fills the pinned stages chunk by chunk on the
// transfer stream and records each chunk's event; the pipeline runs chunk k once its event has been
// recorded (a wait on an unrecorded event would not wait).  The copier never waits on the calling
// thread: it runs through every chunk, so join() always returns.
class ChunkFeed {
 public:
  // chunk k: bytes hoff[cuts[k]] .. hoff[cuts[k + 1]] of src to the same offsets of ddata
  ChunkFeed(DevCtx& d, uint8_t* ddata, const uint8_t* src, const std::vector<uint64_t>& hoff, const std::vector<size_t>& cuts)
      : d_(d), copied_(std::chrono::steady_clock::now()), copier_([this, ddata, src, &hoff, &cuts] {
          const size_t nch = cuts.size() - 1;
          hipError_t e = hipSetDevice(d_.hip_id);
          for (size_t k = 0; k < nch && e == hipSuccess; ++k) {
            const uint64_t b0 = hoff[cuts[k]], b1 = hoff[cuts[k + 1]];
            e = d_.stager->put(ddata + b0, src + b0, b1 - b0);
            if (e == hipSuccess) e = d_.stager->flush();
            if (e == hipSuccess) e = hipEventRecord(d_.ev_chunk[k], d_.xfer);
            if (k + 1 == nch) copied_ = std::chrono::steady_clock::now();
            std::lock_guard<std::mutex> g(mu_);
            if (e == hipSuccess) recorded_ = k + 1;
            else copy_err_ = e;
            cv_.notify_all();
          }
        }) {}
  ~ChunkFeed() { join(); }
  // returns once chunk k's bytes are on their way and the call's stream waits for them
  int wait(size_t k) {
    {
      std::unique_lock<std::mutex> g(mu_);
      cv_.wait(g, [&] { return recorded_ > k || copy_err_ != hipSuccess; });
      if (recorded_ <= k) return set_err(NWC_ERR_DEVICE, "message copy: %s", hipGetErrorString(copy_err_));
    }
    const hipError_t e = hipStreamWaitEvent(d_.stream, d_.ev_chunk[k], 0);
    if (e != hipSuccess) return set_err(NWC_ERR_DEVICE, "hipStreamWaitEvent: %s", hipGetErrorString(e));
    return 0;
  }
  // whether they are, without waiting
  bool queued(size_t k) {
    std::lock_guard<std::mutex> g(mu_);
    return recorded_ > k;
  }
  void join() {
    if (copier_.joinable()) copier_.join();
  }
  // when the last chunk's copy was queued (read after join())
  std::chrono::steady_clock::time_point copied() const { return copied_; }

 private:
  DevCtx& d_;
  std::mutex mu_;
  std::condition_variable cv_;
  size_t recorded_ = 0;   // chunks [0, recorded_) have their event recorded
  hipError_t copy_err_ = hipSuccess;
  std::chrono::steady_clock::time_point copied_;
  std::thread copier_;   // last: it starts in the constructor and uses the members above
};

// What the _ex entries add to a call, as device pointers (all null: the plain call).  gc_rounds
// and targets (80-byte records, MSG_TARGET_STRIDE) give message i its own Core state; key is the
// signer's key record, and with it vote_sigs (m x 64 B) and voted (m bytes) are written by
// k_vote_msgs behind the codes; kinds (m bytes) is the device entry's twin of the host's kinds.
// views (m x 160 B, nwc_msg_view), body (16-byte aligned, body_cap bytes) and body_used (u64) are
// what the _view entries add: k_message_views writes them behind the codes, once per call.
struct MsgEx {
  const uint64_t* gc_rounds = nullptr;
  const uint8_t* targets = nullptr;
  const nwc::SignKey* key = nullptr;
  uint8_t* vote_sigs = nullptr;
  uint8_t* voted = nullptr;
  uint8_t* kinds = nullptr;
  uint8_t* views = nullptr;
  uint8_t* body = nullptr;
  uint64_t body_cap = 0;
  uint64_t* body_used = nullptr;
};

// Device part of nwc_sanitize_messages: messages in HBM (ddata 4-byte aligned with >= 16 bytes
// of readable padding, doff device u64[m+1] relative to ddata, `total` bytes), parsed as the
// chunks cuts[k] .. cuts[k+1] (whole messages).  `feed`, when given, is the host path's copies:
// feed->wait(k) returns once chunk k's bytes are on their way and stream s waits for them;
// feed->queued(k) tells without waiting whether they are, and chunk k's parse is then queued
// before the host waits for chunk k - 1's count.  The chunks share one vote-slot counter, so the
// votes of the chunks parsed so far are contiguous; after each parse the host reads the count and
// launches those votes' leaves on the side stream beside the next chunk's parse, and the rest
// after the last chunk.  (Measured and removed in round 6: leaves behind the parses on one stream,
// leaves in whole comb rounds, per-launch list passes, each parse queued only after the previous
// count -- profiles/r05/wire_host.md, ab_wire_modes.txt, ab_wire_defer_lists.txt.)
// The strict equations (headers' and votes' own signatures) of all chunks but the last run while
// the last one crosses PCIe; the header digests and the final codes run once over all m messages.
struct MsgPipeline {
  DevCtx& d;
  const hipStream_t s;               // the parse stream: the call's stream
  const std::vector<size_t>& cuts;
  const size_t nch;
  ChunkFeed* const feed;
  MsgSchedule sch{};
  // the leaf stream when chunks overlap: the side stream, which has a hardware queue of its own
  // (GPU_MAX_HW_QUEUES = 4: a stream created later shared the transfer stream's queue, and its
  // leaves waited behind the markers of the in-flight copies, profiles/r05/wire_host.md)
  hipStream_t ls = nullptr;
  nwc::MsgArgs a{};                  // the whole call's arrays
  MsgEx ex{};                        // per-message state and votes (nwc_sanitize_messages_ex)
  uint64_t vt = 0;                   // vote slots
  nwc::SignRecs sr{};                // vote v's record at index v
  nwc::SignRecs srs{};               // the strict equations' records (message i at index i)
  uint64_t* sbits = nullptr;         // the strict equations' verdict words
  uint64_t* lbits = nullptr;         // the leaves' verdict words
  const uint64_t* doff = nullptr;
  uint8_t* ddigests = nullptr;
  int32_t* dcodes = nullptr;
  uint32_t* nv_host = nullptr;       // pinned: the count copies stay asynchronous
  nwc::Committee cm{};
  nwc::CommitteeCfg cc{};
  size_t first_lds = 0;
  struct HoldLists {
    DevCtx& d;
    ~HoldLists() { d.hold_lists = false; }
  } hold;

  uint64_t launched = 0;     // votes [0, launched) have their leaf launch queued
  // ysplit: votes [owed_lo, owed_hi) have had their leaves but not their sign tests yet; those run
  // in the first blocks of the next chunk's leaf launch (k_verify_comb_y_sign), so their
  // latency-bound chain overlaps its comb sums, or alone before a list pass needs their words
  uint64_t owed_lo = 0, owed_hi = 0;
  bool pending = false;      // deferred leaf launches whose list passes have not been queued
  bool list_dirty = false;   // a strict launch on ls has reused the uncached list since its reset
  size_t strict_done = 0;    // messages [0, strict_done) have their strict launch queued
  size_t queued = 0;         // chunks whose parse is queued
  uint64_t nv = 0;           // votes parsed so far, as of the last count read

  // NWC_HOST_TIMING: host-side stamps of the steps (which call waits on what)
  const bool timing = settings().host_timing;
  std::chrono::steady_clock::time_point tm0;
  std::vector<std::pair<const char*, double>> marks;
  void mark(const char* what) {
    if (timing) marks.emplace_back(what, std::chrono::duration<double>(std::chrono::steady_clock::now() - tm0).count() * 1e3);
  }

  MsgPipeline(DevCtx& d, hipStream_t s, const std::vector<size_t>& cuts, ChunkFeed* feed)
      : d(d), s(s), cuts(cuts), nch(cuts.size() - 1), feed(feed), hold{d} {}

  // The schedule, the message arena, its memsets and the deferred list's reset.
  int setup(const uint8_t* ddata, const uint64_t* doff_, size_t m, uint64_t total, uint64_t gc_round,
            const uint8_t* vote_target, int32_t* dcodes_, uint8_t* ddigests_, uint32_t* drec, const MsgEx& ex_ = {}) {
    if (int rc = ensure_verify_tables(d)) return rc;
    ex = ex_;
    vt = nwc::plan::vote_slots(total, nch);
    if (!vt) return set_err(NWC_ERR_ARG, "too many vote slots in one call");
    sch = nwc::plan::schedule(nch, deferrable_list(d), g_cm_is_config.load(), settings());
    // a call that signs votes publishes the digests (the votes' ids) whether or not its caller takes them
    const bool own_digests = ex.key && !ddigests_;
    const nwc::plan::MsgArena L = nwc::plan::msg_arena(m, total, vt, sch.ysplit, !drec, own_digests);
    if (int rc = ensure_idle(d, d.msg_arena, L.bytes, &s, L.bytes / 4 + (1 << 20))) return rc;
    uint8_t* const base = d.msg_arena;
    doff = doff_;
    dcodes = dcodes_;
    ddigests = own_digests ? arena_at<uint8_t>(base, L.digests) : ddigests_;
    a.data = ddata;
    a.offsets = doff;
    a.m = m;
    a.gc_round = gc_round;
    a.hashbuf = arena_at<uint8_t>(base, L.hashbuf);
    a.eq_msg = arena_at<uint8_t>(base, L.eq_msg);
    a.eq_pk = arena_at<uint8_t>(base, L.eq_pk);
    a.eq_sig = arena_at<uint8_t>(base, L.eq_sig);
    a.cdig = arena_at<uint8_t>(base, L.cdig);
    a.v_pk = arena_at<uint8_t>(base, L.v_pk);
    a.v_sig = arena_at<uint8_t>(base, L.v_sig);
    a.v_msg = arena_at<uint32_t>(base, L.v_msg);
    a.v_total = arena_at<uint32_t>(base, L.v_total);
    a.v_cap = vt;
    a.hmatch = arena_at<uint32_t>(base, L.hmatch);
    a.rec = drec ? drec : arena_at<uint32_t>(base, L.rec);
    a.rec_n = arena_at<uint32_t>(base, L.rec_n);
    sbits = arena_at<uint64_t>(base, L.sbits);
    lbits = arena_at<uint64_t>(base, L.lbits);
    if (sch.ysplit) {
      sr = {arena_at<uint32_t>(base, L.sr_x), arena_at<uint32_t>(base, L.sr_z), arena_at<uint32_t>(base, L.sr_p),
            arena_at<uint32_t>(base, L.sr_meta)};
      srs = {arena_at<uint32_t>(base, L.srs_x), arena_at<uint32_t>(base, L.srs_z), arena_at<uint32_t>(base, L.srs_p),
             arena_at<uint32_t>(base, L.srs_meta)};
      HIP_TRY(hipMemsetAsync(lbits, 0, 8 * ((vt + 63) / 64), s));   // the sign and list passes OR into it
      HIP_TRY(hipMemsetAsync(sbits, 0, 8 * ((m + 63) / 64), s));
    }
    a.digests = ddigests;
    if (vote_target) {
      a.target.enabled = 1;
      std::memcpy(a.target.id, vote_target, 32);
      std::memcpy(&a.target.round, vote_target + 32, 8);
      std::memcpy(a.target.origin, vote_target + 40, 32);
    }
    if (int rc = d.ensure_pinned(NWC_PINNED_STAGE_MAX)) return rc;
    if (nch > nwc::plan::stage_chunk_limit()) return set_err(NWC_ERR_ARG, "too many chunks");
    nv_host = reinterpret_cast<uint32_t*>(d.pinned.get() + nwc::plan::STAGE_COUNTS_AT);
    if (int rc = ensure_events(d.ev_cnt, nch)) return rc;
    ls = sch.chunked ? d.side : s;
    if (sch.defer) {
      if (int rc = ensure_scratch(d, 0, vt)) return rc;
      d.hold_lists = true;
      HIP_TRY(hipStreamWaitEvent(ls, d.scratch_free, 0));
      HIP_TRY(hipMemsetAsync(d.uc_count, 0, sizeof(uint32_t), ls));
    }
    HIP_TRY(hipMemsetAsync(a.v_total, 0, 4, s));
    HIP_TRY(hipMemsetAsync(a.v_msg, 0, 4 * vt, s));
    cm = committee_of(d);
    cc = nwc::CommitteeCfg{d.cc_stakes, d.cc_worker_off, d.cc_worker_ids, d.cc_quorum, d.cc_n};
    first_lds = 4 * (size_t)std::max<uint32_t>(1, std::min<uint32_t>(d.cc_n, nwc::MSG_MAX_COMMITTEE));
    tm0 = std::chrono::steady_clock::now();
    return 0;
  }

  // the leaf launch of votes [launched, upto) on the leaf stream
  int leaves(uint64_t upto, bool deferred) {
    if (upto <= launched) return 0;
    if (deferred && list_dirty) {
      HIP_TRY(hipMemsetAsync(d.uc_count, 0, sizeof(uint32_t), ls));
      list_dirty = false;
    }
    const uint64_t v0 = launched;
    const bool y = deferred && sch.ysplit;
    const nwc::SignPass sp{sr, owed_lo, owed_hi - owed_lo, lbits, comb_sign_blocks(d, owed_hi - owed_lo)};
    const nwc::SignRecs srl = sign_recs_at(sr, (int64_t)v0);
    if (int rc = launch_verify(d, {.msgs = a.cdig, .msg_index = a.v_msg + v0, .pks = a.v_pk + 32 * v0, .sigs = a.v_sig + 64 * v0,
                                   .n = upto - v0, .out_words = lbits + v0 / 64, .stream = ls,
                                   .flags = deferred ? LV_DEFER_LIST : 0, .list_base = v0, .sign_recs = y ? &srl : nullptr,
                                   .sign_pass = y ? &sp : nullptr}))
      return rc;
    if (y) {
      owed_lo = v0;
      owed_hi = upto;
    }
    pending = pending || deferred;
    launched = upto;
    mark("leaves queued");
    return 0;
  }

  // the list passes of the deferred leaves so far (they OR the uncached votes' bits into the words
  // the comb or sign kernels wrote), after the sign tests still owed
  int finish() {
    if (owed_hi > owed_lo) {
      if (int rc = launch_comb_sign(d, sr, owed_lo, owed_hi - owed_lo, lbits, ls)) return rc;
      owed_lo = owed_hi;
    }
    if (!pending) return 0;
    pending = false;
    return finish_deferred_list(d, a.cdig, a.v_msg, 0, a.v_pk, a.v_sig, launched, 0, lbits, ls);
  }

  // the strict equations (headers' and votes' own signatures) of messages [c0, c1): list-free on
  // the parse stream (MsgSchedule::strict_y), or on the leaf stream after the list passes (the
  // strict launch reuses the list)
  int strict(size_t c0, size_t c1) {
    if (c1 <= c0) return 0;
    if (sch.strict_y) {
      const uint64_t n = c1 - c0;
      const nwc::VerifyArgs va{a.eq_msg + 32 * c0, nullptr, 1, a.eq_pk + 32 * c0, a.eq_sig + 64 * c0, sbits + c0 / 64,
                               n, 1, d.base_table, d.base24, d.scratch, d.fb_list, d.fb_count, 0u, cm};
      const nwc::CombArgs ca{nullptr, nullptr, d.comb_base, d.comb16, nullptr, 0};
      const unsigned gy = (unsigned)std::min<uint64_t>((n + 255) / 256, 60000);
      hipLaunchKernelGGL(nwc::k_verify_comb_y, dim3(gy), dim3(256), 0, s, va, ca, sign_recs_at(srs, (int64_t)c0));
      HIP_TRY(hipGetLastError());
      return launch_comb_sign(d, srs, c0, n, sbits, s);
    }
    if (int rc = finish()) return rc;
    list_dirty = true;
    return launch_verify(d, {.msgs = a.eq_msg + 32 * c0, .msg_stride = 1, .pks = a.eq_pk + 32 * c0, .sigs = a.eq_sig + 64 * c0,
                             .n = c1 - c0, .strict = 1, .out_words = sbits + c0 / 64, .stream = ls});
  }

  // the next chunk's parse on the parse stream, and the copy of the vote count so far
  int queue_parse() {
    const size_t k = queued++;
    if (feed)
      if (int rc = feed->wait(k)) return rc;
    mark("chunk ready");
    const size_t c0 = cuts[k];
    nwc::MsgArgs ak = a;
    ak.offsets = doff + c0;
    ak.m = cuts[k + 1] - c0;
    ak.hashbuf = a.hashbuf + 128 * c0;   // the message's slot: aligned data offset + 128 x (call-wide index)
    ak.eq_msg = a.eq_msg + 32 * c0;
    ak.eq_pk = a.eq_pk + 32 * c0;
    ak.eq_sig = a.eq_sig + 64 * c0;
    ak.cdig = a.cdig + 32 * c0;
    ak.msg_base = (uint32_t)c0;
    ak.hmatch = a.hmatch + c0;
    ak.rec = a.rec + 4 * c0;
    ak.rec_n = a.rec_n + c0;
    ak.digests = ddigests ? ddigests + 32 * c0 : nullptr;
    if (ex.gc_rounds || ex.targets) {
      // the chunk's own state from its first message, as its offsets
      const nwc::MsgOwnState own{ex.gc_rounds ? ex.gc_rounds + c0 : nullptr,
                                 ex.targets ? ex.targets + nwc::plan::MSG_TARGET_STRIDE * c0 : nullptr};
      hipLaunchKernelGGL(nwc::k_parse_messages_own, dim3((unsigned)ak.m), dim3(64), first_lds, s, ak, cm, cc, own);
    } else {
      hipLaunchKernelGGL(nwc::k_parse_messages, dim3((unsigned)ak.m), dim3(64), first_lds, s, ak, cm, cc);
    }
    HIP_TRY(hipGetLastError());
    if (nch > 1) {
      // the next chunk's votes from a 64-slot boundary: every leaf launch starts on its own
      // verdict word (the skipped slots repeat the last vote; their leaves are never read)
      hipLaunchKernelGGL(nwc::k_align_slots, dim3(1), dim3(64), 0, s, a.v_total, (uint32_t)vt, a.v_pk, a.v_sig,
                         a.v_msg);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(nv_host + k, a.v_total, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(d.ev_cnt[k], s));
    mark("parse queued");
    return 0;
  }

  // Every chunk's parse, and for a chunked call the leaves of all chunks but the last and the
  // early strict launch.
  int run_parses() {
    if (int rc = queue_parse()) return rc;
    for (size_t k = 0; k < nch; ++k) {
      // the next chunk's parse goes in before this chunk's count is awaited when its copy is already
      // queued (no wait on the copier): it then follows this parse on the GPU without a host round
      // trip in between
      if (queued < nch && (!feed || feed->queued(queued)))
        if (int rc = queue_parse()) return rc;
      if (!sch.chunked) continue;
      // the votes parsed so far on the leaf stream; the next chunk's copy goes on in the copier
      // thread meanwhile, and its parse runs beside these leaves
      HIP_TRY(hipEventSynchronize(d.ev_cnt[k]));
      nv = std::min<uint64_t>(nv_host[k], vt);
      mark("count");
      HIP_TRY(hipStreamWaitEvent(ls, d.ev_cnt[k], 0));
      // (the last leaf launch then holds only the last chunk's votes)
      if (k + 1 < nch)
        if (int rc = leaves(nv, sch.defer)) return rc;
      if (k == sch.strict_at) {
        if (int rc = strict(0, cuts[k + 1])) return rc;
        strict_done = cuts[k + 1];
      }
      if (queued == k + 1 && queued < nch)
        if (int rc = queue_parse()) return rc;
    }
    return 0;
  }

  // after the last chunk's count: the header digests, the last leaves and the remaining strict
  // equations; the parse stream then waits for the leaf stream
  int run_chunked() {
    // the Header::digest checks once, beside the last leaves (latency-bound: ~0.2 ms for any
    // number of messages, so not per chunk)
    hipLaunchKernelGGL(nwc::k_header_digests, dim3((unsigned)((a.m + 255) / 256)), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    if (sch.ysplit) {
      // the last chunk's leaves deferred as well (a fresh list: the strict launch reused it),
      // their sign tests, then the list passes and the remaining strict equations
      if (int rc = leaves(nv, true)) return rc;
      if (int rc = strict(strict_done, a.m)) return rc;
      if (int rc = finish()) return rc;   // (strict_y: the strict launches left the leaf stream's passes)
    } else {
      if (int rc = strict(strict_done, a.m)) return rc;
      if (int rc = leaves(nv, false)) return rc;
    }
    HIP_TRY(hipEventRecord(d.ev_msg, ls));
    HIP_TRY(hipStreamWaitEvent(s, d.ev_msg, 0));
    return 0;
  }

  // one chunk: the strict launch (it needs no count) queued before the host waits for the
  // count, the Header::digest checks beside the leaves on the side stream
  int run_single() {
    if (int rc = launch_verify(d, {.msgs = a.eq_msg, .msg_stride = 1, .pks = a.eq_pk, .sigs = a.eq_sig, .n = a.m, .strict = 1,
                                   .out_words = sbits, .stream = s}))
      return rc;
    HIP_TRY(hipEventRecord(d.ev_fork, s));
    HIP_TRY(hipStreamWaitEvent(d.side, d.ev_fork, 0));
    hipLaunchKernelGGL(nwc::k_header_digests, dim3((unsigned)((a.m + 255) / 256)), dim3(256), 0, d.side, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(d.ev_msg, d.side));
    HIP_TRY(hipEventSynchronize(d.ev_cnt[0]));
    if (int rc = leaves(std::min<uint64_t>(nv_host[0], vt), false)) return rc;
    HIP_TRY(hipStreamWaitEvent(s, d.ev_msg, 0));
    return 0;
  }

  // the whole call after setup(), up to the codes in dcodes (queued on s, not awaited)
  int run() {
    if (int rc = run_parses()) return rc;
    if (int rc = sch.chunked ? run_chunked() : run_single()) return rc;
    hipLaunchKernelGGL(nwc::k_finalize_messages, dim3((unsigned)((a.m + 255) / 256)), dim3(256), 0, s, a.rec,
                       a.rec_n, a.hmatch, sbits, lbits, (uint64_t)a.m, dcodes);
    HIP_TRY(hipGetLastError());
    if (ex.key) {
      // Vote::new for the headers whose final code is Ok, once, over the whole call
      hipLaunchKernelGGL(nwc::k_vote_msgs, dim3((unsigned)a.m), dim3(64), 0, s, ex.key, (const nwc::ge_niels*)d.sign_table, dcodes,
                         a.rec, ddigests, a.eq_pk, a.data, doff, (uint64_t)a.m, ex.vote_sigs, ex.voted);
      HIP_TRY(hipGetLastError());
    }
    if (ex.kinds) {
      hipLaunchKernelGGL(nwc::k_msg_kinds, dim3((unsigned)((a.m + 255) / 256)), dim3(256), 0, s, a.rec, (uint64_t)a.m, ex.kinds);
      HIP_TRY(hipGetLastError());
    }
    if (ex.views) {
      // the decoded views, once, over the whole call: one wave per message, the body's allocator from zero
      HIP_TRY(hipMemsetAsync(ex.body_used, 0, 8, s));
      const nwc::ViewOut vo{reinterpret_cast<uint32_t*>(ex.views), ex.body, ex.body_cap,
                            reinterpret_cast<unsigned long long*>(ex.body_used)};
      hipLaunchKernelGGL(nwc::k_message_views, dim3((unsigned)a.m), dim3(64), 0, s, a, cm, (const int32_t*)dcodes, vo);
      HIP_TRY(hipGetLastError());
    }
    mark("final queued");
    if (timing && nch > 1) {
      std::string line;
      for (const auto& mk : marks) line += std::string(" ") + mk.first + "@" + std::to_string(mk.second).substr(0, 5);
      std::fprintf(stderr, "nwc sanitize steps:%s\n", line.c_str());
    }
    return 0;
  }
};

int sanitize_dev(DevCtx& d, const uint8_t* ddata, const uint64_t* doff, size_t m, uint64_t total,
                 const std::vector<size_t>& cuts, uint64_t gc_round, const uint8_t* vote_target, int32_t* dcodes,
                 uint8_t* ddigests, uint32_t* drec, hipStream_t s, ChunkFeed* feed = nullptr, const MsgEx& ex = {}) {
  MsgPipeline p(d, s, cuts, feed);
  if (int rc = p.setup(ddata, doff, m, total, gc_round, vote_target, dcodes, ddigests, drec, ex)) return rc;
  return p.run();
}

// What an _ex call adds to a host call, as host pointers (key: the device's key record): the
// per-message state goes up with the offsets, the votes come back with the codes.
struct HostEx {
  const uint64_t* gc_rounds = nullptr;
  const uint8_t* targets = nullptr;
  const nwc::SignKey* key = nullptr;
  uint8_t* vote_sigs = nullptr;
  uint8_t* voted = nullptr;
  // nwc_sanitize_messages_view: the records (m x 160 B), then the used part of the body, come back
  // behind the codes
  uint8_t* views = nullptr;
  uint8_t* body = nullptr;
  uint64_t* body_used = nullptr;
};

// One device's share of a host call: stages the messages (small batches in one copy, large ones
// chunk by chunk through a ChunkFeed), runs the pipeline and reads the codes, kinds and digests back.
int sanitize_range(int di, const uint8_t* data, const uint64_t* offsets, size_t m, uint64_t gc_round,
                   const uint8_t* vote_target, int32_t* codes, uint8_t* digests32, uint8_t* kinds, const HostEx& hx = {}) {
  if (m == 0) return 0;
  const uint64_t base = offsets[0], total = offsets[m] - base;
  DevCtx& d = *ctx(di);
  std::lock_guard<std::mutex> lk(d.mu);
  HIP_TRY(hipSetDevice(d.hip_id));
  if (int rc = ensure_verify_tables(d)) return rc;
  if (!d.cc_stakes) return set_err(NWC_ERR_NOT_INIT, "nwc_set_committee_config has not been called");
  // staging area (the arena): message bytes, offsets, codes, records, digests
  const bool own_state = hx.gc_rounds || hx.targets;
  const nwc::plan::CallArena L = nwc::plan::call_arena(m, total, own_state, hx.key != nullptr, hx.views != nullptr);
  if (int rc = d.ensure_arena(L.bytes)) return rc;
  if (hx.key)
    if (int rc = ensure_sign_table(d)) return rc;
  uint8_t* const arena = d.arena;
  uint8_t* ddata = arena_at<uint8_t>(arena, L.data);
  uint64_t* doff = arena_at<uint64_t>(arena, L.offsets);
  int32_t* dcodes = arena_at<int32_t>(arena, L.codes);
  uint32_t* drec = arena_at<uint32_t>(arena, L.rec);
  uint8_t* ddig = (digests32 || hx.key) ? arena_at<uint8_t>(arena, L.digests) : nullptr;
  MsgEx ex;
  ex.key = hx.key;
  if (hx.key) {
    ex.vote_sigs = arena_at<uint8_t>(arena, L.vote_sigs);
    ex.voted = arena_at<uint8_t>(arena, L.voted);
  }
  if (hx.views) {
    ex.views = arena_at<uint8_t>(arena, L.views);
    ex.body = arena_at<uint8_t>(arena, L.body);
    ex.body_cap = nwc::plan::view_body_bound(total, m);
    ex.body_used = arena_at<uint64_t>(arena, L.body_used);
  }
  std::vector<uint64_t> hoff(m + 1);
  for (size_t i = 0; i <= m; ++i) hoff[i] = offsets[i] - base;
  // The chunks share the message offsets (uploaded first, relative to ddata) and the message arena
  // (the pipeline parses them in stream order).
  const bool staged = nwc::plan::staged(total);
  const std::vector<size_t> cuts = nwc::plan::message_cuts(hoff.data(), m, settings());
  const size_t nch = cuts.size() - 1;
  HIP_TRY(hipMemsetAsync(ddata + total, 0, 16, d.stream));
  // the offsets through pinned memory when they fit beside the chunk counts (a pageable source
  // makes the copy wait for the host)
  if (nwc::plan::stage_holds_offsets(m, NWC_PINNED_STAGE_MAX)) {
    if (int rc = d.ensure_pinned(NWC_PINNED_STAGE_MAX)) return rc;
    uint8_t* const ph = static_cast<uint8_t*>(d.pinned) + nwc::plan::STAGE_OFFSETS_AT;
    std::memcpy(ph, hoff.data(), 8 * (m + 1));
    HIP_TRY(hipMemcpyAsync(doff, ph, 8 * (m + 1), hipMemcpyHostToDevice, d.stream));
  } else {
    HIP_TRY(hipMemcpyAsync(doff, hoff.data(), 8 * (m + 1), hipMemcpyHostToDevice, d.stream));
  }
  // the per-message state with the offsets: on the call's stream, before the first parse
  if (hx.gc_rounds) {
    uint64_t* dgc = arena_at<uint64_t>(arena, L.gc_rounds);
    HIP_TRY(hipMemcpyAsync(dgc, hx.gc_rounds, 8 * m, hipMemcpyHostToDevice, d.stream));
    ex.gc_rounds = dgc;
  }
  if (hx.targets) {
    uint8_t* dtg = arena_at<uint8_t>(arena, L.targets);
    HIP_TRY(hipMemcpyAsync(dtg, hx.targets, nwc::plan::MSG_TARGET_STRIDE * m, hipMemcpyHostToDevice, d.stream));
    ex.targets = dtg;
  }
  if (!staged) {
    HIP_TRY(hipMemcpyAsync(ddata, data + base, total, hipMemcpyHostToDevice, d.stream));
    if (int rc = sanitize_dev(d, ddata, doff, m, total, {0, m}, gc_round, vote_target, dcodes, ddig, drec, d.stream, nullptr, ex))
      return rc;
  } else {
    if (int rc = ensure_stager(d)) return rc;
    if (int rc = ensure_events(d.ev_chunk, nch)) return rc;
    // the copies wait for every launch that may still read the arena
    HIP_TRY(hipEventRecord(d.ev_fork, d.stream));
    HIP_TRY(hipStreamWaitEvent(d.xfer, d.ev_fork, 0));
    d.stager->reset();
    const auto tm0 = std::chrono::steady_clock::now();
    ChunkFeed feed(d, ddata, data + base, hoff, cuts);
    int rc = sanitize_dev(d, ddata, doff, m, total, cuts, gc_round, vote_target, dcodes, ddig, drec, d.stream, &feed, ex);
    feed.join();
    if (rc) {
      (void)hipStreamSynchronize(d.xfer);   // no copy still writes the arena when the call returns
      return rc;
    }
    if (settings().host_timing) {
      HIP_TRY(hipStreamSynchronize(d.stream));
      const auto tm1 = std::chrono::steady_clock::now();
      const auto tm_copied = feed.copied();
      std::fprintf(stderr, "nwc sanitize: %zu messages, %.1f MB in %zu chunks: copies queued after %.2f ms, pipeline done %.2f ms later\n",
                   m, total / 1e6, nch, std::chrono::duration<double>(tm_copied - tm0).count() * 1e3,
                   std::chrono::duration<double>(tm1 - tm_copied).count() * 1e3);
    }
  }
  HIP_TRY(hipMemcpyAsync(codes, dcodes, 4 * m, hipMemcpyDeviceToHost, d.stream));
  std::vector<uint32_t> rec;
  if (kinds) {
    rec.resize(4 * m);
    HIP_TRY(hipMemcpyAsync(rec.data(), drec, 16 * m, hipMemcpyDeviceToHost, d.stream));
  }
  if (digests32) HIP_TRY(hipMemcpyAsync(digests32, ddig, 32 * m, hipMemcpyDeviceToHost, d.stream));
  if (hx.key) {
    HIP_TRY(hipMemcpyAsync(hx.vote_sigs, ex.vote_sigs, 64 * m, hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(hipMemcpyAsync(hx.voted, ex.voted, m, hipMemcpyDeviceToHost, d.stream));
  }
  if (hx.views) {
    HIP_TRY(hipMemcpyAsync(hx.views, ex.views, nwc::plan::MSG_VIEW_BYTES * m, hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(hipMemcpyAsync(hx.body_used, ex.body_used, 8, hipMemcpyDeviceToHost, d.stream));
  }
  HIP_TRY(hipStreamSynchronize(d.stream));
  if (kinds)
    for (size_t i = 0; i < m; ++i) kinds[i] = (uint8_t)rec[4 * i];
  if (hx.views && *hx.body_used) {
    // only what the allocator handed out, never the whole capacity
    const uint64_t used = std::min<uint64_t>(*hx.body_used, ex.body_cap);
    HIP_TRY(hipMemcpyAsync(hx.body, ex.body, used, hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
  }
  return 0;
}

}  // namespace

extern "C" {

int nwc_sanitize_messages(const uint8_t* data, const uint64_t* offsets, size_t m, uint64_t gc_round,
                          const uint8_t* vote_target, int32_t* codes, uint8_t* digests32, uint8_t* kinds) {
  if (int rc = require_init()) return rc;
  if (m == 0) return 0;
  if (!data || !offsets || !codes) return set_err(NWC_ERR_ARG, "null buffer");
  for (size_t i = 0; i < m; ++i)
    if (offsets[i + 1] < offsets[i]) return set_err(NWC_ERR_ARG, "offsets not monotone at %zu", i);
  // messages are independent: contiguous ranges per device, one host thread each
  return shard(m, [&](int di, uint64_t lo, uint64_t hi) -> int {
    return sanitize_range(di, data, offsets + lo, hi - lo, gc_round, vote_target, codes + lo,
                          digests32 ? digests32 + 32 * lo : nullptr, kinds ? kinds + lo : nullptr);
  });
}

int nwc_dev_sanitize_messages(const void* d_data, const void* d_offsets, uint64_t m, uint64_t total,
                              uint64_t gc_round, const uint8_t* vote_target, void* d_codes, void* d_digests32,
                              void* stream) {
  if (int rc = require_init()) return rc;
  if (m == 0) return 0;
  if (!d_data || !d_offsets || !d_codes) return set_err(NWC_ERR_ARG, "null buffer");
  if ((reinterpret_cast<uintptr_t>(d_data) & 3) != 0) return set_err(NWC_ERR_ARG, "d_data must be 4-byte aligned");
  DevCtx& d = *ctx(t_dev < (int)g_devs.size() ? t_dev : 0);
  std::lock_guard<std::mutex> lk(d.mu);
  HIP_TRY(hipSetDevice(d.hip_id));
  if (!d.cc_stakes) return set_err(NWC_ERR_NOT_INIT, "nwc_set_committee_config has not been called");
  return sanitize_dev(d, static_cast<const uint8_t*>(d_data), static_cast<const uint64_t*>(d_offsets), m, total,
                      {0, (size_t)m}, gc_round, vote_target, static_cast<int32_t*>(d_codes), static_cast<uint8_t*>(d_digests32),
                      nullptr, stream ? static_cast<hipStream_t>(stream) : d.stream);
}

int nwc_sanitize_messages_ex(const uint8_t* data, const uint64_t* offsets, size_t m, const uint64_t* gc_rounds,
                             uint64_t gc_round, const uint8_t* vote_targets80, const uint8_t* vote_target, void* signer,
                             int32_t* codes, uint8_t* digests32, uint8_t* kinds, uint8_t* vote_sigs, uint8_t* voted) {
  // on an error < 0 every vote output is zero
  auto fail = [&](int rc) {
    if (signer && m && vote_sigs) std::memset(vote_sigs, 0, 64 * m);
    if (signer && m && voted) std::memset(voted, 0, m);
    return rc;
  };
  if (signer && (!vote_sigs || !voted)) return fail(set_err(NWC_ERR_ARG, "a signer needs vote_sigs and voted"));
  if (m == 0) return 0;
  if (int rc = require_init()) return fail(rc);
  if (!data || !offsets || !codes) return fail(set_err(NWC_ERR_ARG, "null buffer"));
  for (size_t i = 0; i < m; ++i)
    if (offsets[i + 1] < offsets[i]) return fail(set_err(NWC_ERR_ARG, "offsets not monotone at %zu", i));
  HostEx hx;
  hx.gc_rounds = gc_rounds;
  hx.targets = vote_targets80;
  if (!signer) {
    // messages are independent: contiguous ranges per device, as nwc_sanitize_messages
    return shard(m, [&](int di, uint64_t lo, uint64_t hi) -> int {
      HostEx h = hx;
      if (h.gc_rounds) h.gc_rounds += lo;
      if (h.targets) h.targets += nwc::plan::MSG_TARGET_STRIDE * lo;
      return sanitize_range(di, data, offsets + lo, hi - lo, gc_round, vote_target, codes + lo,
                            digests32 ? digests32 + 32 * lo : nullptr, kinds ? kinds + lo : nullptr, h);
    });
  }
  // with a signer: whole, on the signer's device (its key record lives there)
  Signer& sg = *static_cast<Signer*>(signer);
  if (!sg.d || !sg.key) return fail(set_err(NWC_ERR_NOT_INIT, "the signer's device context was shut down"));
  int di = -1;
  for (size_t k = 0; k < g_devs.size(); ++k)
    if (g_devs[k].get() == sg.d) di = (int)k;
  if (di < 0) return fail(set_err(NWC_ERR_ARG, "the signer's device is not initialised"));
  hx.key = sg.key;
  hx.vote_sigs = vote_sigs;
  hx.voted = voted;
  const int rc = sanitize_range(di, data, offsets, m, gc_round, vote_target, codes, digests32, kinds, hx);
  return rc < 0 ? fail(rc) : rc;
}

int nwc_dev_sanitize_messages_ex(const void* d_data, const void* d_offsets, uint64_t m, uint64_t total,
                                 const void* d_gc_rounds, uint64_t gc_round, const void* d_vote_targets80,
                                 const uint8_t* vote_target, void* signer, void* d_codes, void* d_digests32, void* d_kinds,
                                 void* d_vote_sigs, void* d_voted, void* stream) {
  if (signer && (!d_vote_sigs || !d_voted)) return set_err(NWC_ERR_ARG, "a signer needs d_vote_sigs and d_voted");
  if (m == 0) return 0;
  if (int rc = require_init()) return rc;
  DevCtx& d = *ctx(t_dev < (int)g_devs.size() ? t_dev : 0);
  std::lock_guard<std::mutex> lk(d.mu);
  HIP_TRY(hipSetDevice(d.hip_id));
  const hipStream_t s = stream ? static_cast<hipStream_t>(stream) : d.stream;
  // on an error < 0 every vote output is zero (queued on the call's stream)
  auto fail = [&](int rc) {
    if (signer) {
      (void)hipMemsetAsync(d_vote_sigs, 0, 64 * m, s);
      (void)hipMemsetAsync(d_voted, 0, m, s);
    }
    return rc;
  };
  if (!d_data || !d_offsets || !d_codes) return fail(set_err(NWC_ERR_ARG, "null buffer"));
  if ((reinterpret_cast<uintptr_t>(d_data) & 3) != 0) return fail(set_err(NWC_ERR_ARG, "d_data must be 4-byte aligned"));
  if ((reinterpret_cast<uintptr_t>(d_gc_rounds) & 7) || (reinterpret_cast<uintptr_t>(d_vote_targets80) & 3))
    return fail(set_err(NWC_ERR_ARG, "d_gc_rounds must be 8-byte and d_vote_targets80 4-byte aligned"));
  if (signer && ((reinterpret_cast<uintptr_t>(d_vote_sigs) & 3) || (reinterpret_cast<uintptr_t>(d_digests32) & 15)))
    return fail(set_err(NWC_ERR_ARG, "with a signer d_vote_sigs must be 4-byte and d_digests32 16-byte aligned"));
  if (!d.cc_stakes) return fail(set_err(NWC_ERR_NOT_INIT, "nwc_set_committee_config has not been called"));
  MsgEx ex;
  ex.gc_rounds = static_cast<const uint64_t*>(d_gc_rounds);
  ex.targets = static_cast<const uint8_t*>(d_vote_targets80);
  ex.kinds = static_cast<uint8_t*>(d_kinds);
  if (signer) {
    Signer& sg = *static_cast<Signer*>(signer);
    if (!sg.d || !sg.key) return fail(set_err(NWC_ERR_NOT_INIT, "the signer's device context was shut down"));
    if (sg.d != &d) return fail(set_err(NWC_ERR_ARG, "the signer lives on another device than the calling thread's"));
    if (int rc = ensure_sign_table(d)) return fail(rc);
    ex.key = sg.key;
    ex.vote_sigs = static_cast<uint8_t*>(d_vote_sigs);
    ex.voted = static_cast<uint8_t*>(d_voted);
  }
  const int rc = sanitize_dev(d, static_cast<const uint8_t*>(d_data), static_cast<const uint64_t*>(d_offsets), m, total,
                              {0, (size_t)m}, gc_round, vote_target, static_cast<int32_t*>(d_codes),
                              static_cast<uint8_t*>(d_digests32), nullptr, s, nullptr, ex);
  return rc < 0 ? fail(rc) : rc;
}

uint64_t nwc_msg_view_body_bound(uint64_t total, uint64_t m) { return nwc::plan::view_body_bound(total, m); }

int nwc_sanitize_messages_view(const uint8_t* data, const uint64_t* offsets, size_t m, const uint64_t* gc_rounds,
                               uint64_t gc_round, const uint8_t* vote_targets80, const uint8_t* vote_target, void* signer,
                               int32_t* codes, uint8_t* digests32, uint8_t* kinds, uint8_t* vote_sigs, uint8_t* voted,
                               void* views, uint8_t* body, size_t body_cap, uint64_t* body_used) {
  if (!views)
    return nwc_sanitize_messages_ex(data, offsets, m, gc_rounds, gc_round, vote_targets80, vote_target, signer, codes, digests32,
                                    kinds, vote_sigs, voted);
  // on an error < 0 every view and every vote output is zero, and no body byte is in use
  auto fail = [&](int rc) {
    if (m) std::memset(views, 0, nwc::plan::MSG_VIEW_BYTES * m);
    if (m && body_used) *body_used = 0;
    if (signer && m && vote_sigs) std::memset(vote_sigs, 0, 64 * m);
    if (signer && m && voted) std::memset(voted, 0, m);
    return rc;
  };
  if (signer && (!vote_sigs || !voted)) return fail(set_err(NWC_ERR_ARG, "a signer needs vote_sigs and voted"));
  if (m == 0) return 0;
  // the argument rules first: nothing is queued for a call that breaks one
  if (!body || !body_used) return fail(set_err(NWC_ERR_ARG, "views need body and body_used"));
  if (!data || !offsets || !codes) return fail(set_err(NWC_ERR_ARG, "null buffer"));
  for (size_t i = 0; i < m; ++i) {
    if (offsets[i + 1] < offsets[i]) return fail(set_err(NWC_ERR_ARG, "offsets not monotone at %zu", i));
    if ((offsets[i + 1] - offsets[i]) >> 32) return fail(set_err(NWC_ERR_ARG, "message %zu is 2^32 bytes or longer", i));
  }
  if (body_cap < nwc::plan::view_body_bound(offsets[m] - offsets[0], m))
    return fail(set_err(NWC_ERR_ARG, "body_cap is below nwc_msg_view_body_bound(total, m)"));
  if (int rc = require_init()) return fail(rc);
  HostEx hx;
  hx.gc_rounds = gc_rounds;
  hx.targets = vote_targets80;
  hx.views = static_cast<uint8_t*>(views);
  hx.body = body;
  hx.body_used = body_used;
  // not sharded: whole on the signer's device, or on the calling thread's
  int di = t_dev < (int)g_devs.size() ? t_dev : 0;
  if (signer) {
    Signer& sg = *static_cast<Signer*>(signer);
    if (!sg.d || !sg.key) return fail(set_err(NWC_ERR_NOT_INIT, "the signer's device context was shut down"));
    di = -1;
    for (size_t k = 0; k < g_devs.size(); ++k)
      if (g_devs[k].get() == sg.d) di = (int)k;
    if (di < 0) return fail(set_err(NWC_ERR_ARG, "the signer's device is not initialised"));
    hx.key = sg.key;
    hx.vote_sigs = vote_sigs;
    hx.voted = voted;
  }
  const int rc = sanitize_range(di, data, offsets, m, gc_round, vote_target, codes, digests32, kinds, hx);
  return rc < 0 ? fail(rc) : rc;
}

int nwc_dev_sanitize_messages_view(const void* d_data, const void* d_offsets, uint64_t m, uint64_t total,
                                   const void* d_gc_rounds, uint64_t gc_round, const void* d_vote_targets80,
                                   const uint8_t* vote_target, void* signer, void* d_codes, void* d_digests32, void* d_kinds,
                                   void* d_vote_sigs, void* d_voted, void* d_views, void* d_body, uint64_t body_cap,
                                   void* d_body_used, void* stream) {
  if (!d_views)
    return nwc_dev_sanitize_messages_ex(d_data, d_offsets, m, total, d_gc_rounds, gc_round, d_vote_targets80, vote_target, signer,
                                        d_codes, d_digests32, d_kinds, d_vote_sigs, d_voted, stream);
  if (signer && (!d_vote_sigs || !d_voted)) return set_err(NWC_ERR_ARG, "a signer needs d_vote_sigs and d_voted");
  if (m == 0) return 0;
  if (!d_body || !d_body_used) return set_err(NWC_ERR_ARG, "d_views needs d_body and d_body_used");
  if ((reinterpret_cast<uintptr_t>(d_views) & 7) || (reinterpret_cast<uintptr_t>(d_body) & 15) ||
      (reinterpret_cast<uintptr_t>(d_body_used) & 7))
    return set_err(NWC_ERR_ARG, "d_views and d_body_used must be 8-byte and d_body 16-byte aligned");
  if (body_cap < nwc::plan::view_body_bound(total, m))
    return set_err(NWC_ERR_ARG, "body_cap is below nwc_msg_view_body_bound(total, m)");
  if (int rc = require_init()) return rc;
  DevCtx& d = *ctx(t_dev < (int)g_devs.size() ? t_dev : 0);
  std::lock_guard<std::mutex> lk(d.mu);
  HIP_TRY(hipSetDevice(d.hip_id));
  const hipStream_t s = stream ? static_cast<hipStream_t>(stream) : d.stream;
  // on an error < 0 every view and every vote output is zero and no body byte is in use (queued on
  // the call's stream)
  auto fail = [&](int rc) {
    (void)hipMemsetAsync(d_views, 0, nwc::plan::MSG_VIEW_BYTES * m, s);
    (void)hipMemsetAsync(d_body_used, 0, 8, s);
    if (signer) {
      (void)hipMemsetAsync(d_vote_sigs, 0, 64 * m, s);
      (void)hipMemsetAsync(d_voted, 0, m, s);
    }
    return rc;
  };
  if (!d_data || !d_offsets || !d_codes) return fail(set_err(NWC_ERR_ARG, "null buffer"));
  if ((reinterpret_cast<uintptr_t>(d_data) & 3) != 0) return fail(set_err(NWC_ERR_ARG, "d_data must be 4-byte aligned"));
  if ((reinterpret_cast<uintptr_t>(d_gc_rounds) & 7) || (reinterpret_cast<uintptr_t>(d_vote_targets80) & 3))
    return fail(set_err(NWC_ERR_ARG, "d_gc_rounds must be 8-byte and d_vote_targets80 4-byte aligned"));
  if (signer && ((reinterpret_cast<uintptr_t>(d_vote_sigs) & 3) || (reinterpret_cast<uintptr_t>(d_digests32) & 15)))
    return fail(set_err(NWC_ERR_ARG, "with a signer d_vote_sigs must be 4-byte and d_digests32 16-byte aligned"));
  if (!d.cc_stakes) return fail(set_err(NWC_ERR_NOT_INIT, "nwc_set_committee_config has not been called"));
  MsgEx ex;
  ex.gc_rounds = static_cast<const uint64_t*>(d_gc_rounds);
  ex.targets = static_cast<const uint8_t*>(d_vote_targets80);
  ex.kinds = static_cast<uint8_t*>(d_kinds);
  ex.views = static_cast<uint8_t*>(d_views);
  ex.body = static_cast<uint8_t*>(d_body);
  ex.body_cap = body_cap;
  ex.body_used = static_cast<uint64_t*>(d_body_used);
  if (signer) {
    Signer& sg = *static_cast<Signer*>(signer);
    if (!sg.d || !sg.key) return fail(set_err(NWC_ERR_NOT_INIT, "the signer's device context was shut down"));
    if (sg.d != &d) return fail(set_err(NWC_ERR_ARG, "the signer lives on another device than the calling thread's"));
    if (int rc = ensure_sign_table(d)) return fail(rc);
    ex.key = sg.key;
    ex.vote_sigs = static_cast<uint8_t*>(d_vote_sigs);
    ex.voted = static_cast<uint8_t*>(d_voted);
  }
  const int rc = sanitize_dev(d, static_cast<const uint8_t*>(d_data), static_cast<const uint64_t*>(d_offsets), m, total,
                              {0, (size_t)m}, gc_round, vote_target, static_cast<int32_t*>(d_codes),
                              static_cast<uint8_t*>(d_digests32), nullptr, s, nullptr, ex);
  return rc < 0 ? fail(rc) : rc;
}

}  // extern "C"
