// The message pipeline's host decisions, with no HIP in them: where a staged batch is cut into
// chunks (message_cuts), how many vote slots a call gets (vote_slots), the layouts of the call
// arena, the message arena and the pinned stage, each written once, and what a call defers and
// where its early strict launch goes (schedule).  sanitizer.h reads these and enqueues;
// tests/cpp/msg_plan_host.cpp runs them on the CPU under the host sanitizers.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "verify_plan.h"

namespace nwc {
namespace plan {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Batches of at least this many bytes cross PCIe through the pinned stages on the transfer stream.
constexpr uint64_t MSG_STAGED_MIN = (uint64_t)4 << 20;
inline bool staged(uint64_t total) { return total >= MSG_STAGED_MIN; }

// Chunks of a call over m messages whose bytes start at hoff[0] == 0 .. hoff[m] == total: chunk k
// is messages [cuts[k], cuts[k + 1]).  Large staged batches (config 3 from the wire: 10 KB per
// certificate) go through the pinned stages in chunks of ~msg_chunk bytes cut on message
// boundaries; chunk k is parsed and verified while chunk k + 1 crosses PCIe.  A batch is cut from
// 4 * min(8 MiB, msg_chunk) bytes up; msg_chunk 0 = one copy, then one pass (A/B).
// Chunk sizes: from 16 MB doubling up to msg_chunk, and never more than half of what remains
// (>= 8 MB, so the last one is <= 16 MB): the first parse starts after a short copy, and the
// work left when the last copy lands (that chunk's parse, leaves and strict equations, the
// codes) is small; each leaf launch costs >= ~0.18 ms whatever its size, so not smaller.
inline std::vector<size_t> message_cuts(const uint64_t* hoff, size_t m, const Settings& st) {
  const uint64_t total = hoff[m], msg_chunk = st.msg_chunk;
  std::vector<size_t> cuts{0};
  const uint64_t lo = std::min<uint64_t>((uint64_t)8 << 20, msg_chunk);
  if (staged(total) && msg_chunk && total >= 4 * lo) {
    uint64_t at = 0, next = std::min<uint64_t>(msg_chunk, 2 * lo);
    while (total - at > 2 * lo) {
      const uint64_t want = std::max(lo, std::min(next, (total - at) / 2));
      // every cut on a multiple of 64 messages: each chunk's strict launch owns its verdict words
      size_t cm = (size_t)(std::lower_bound(hoff, hoff + m + 1, at + want) - hoff) & ~(size_t)63;
      if (cm <= cuts.back()) cm = cuts.back() + 64;
      if (cm >= m) break;
      cuts.push_back(cm);
      at = hoff[cm];
      next = std::min<uint64_t>(msg_chunk, 2 * next);
    }
  }
  cuts.push_back(m);
  // Post-condition: cuts.front() == 0, cuts.back() == m, strictly increasing, every interior cut a
  // multiple of 64.  (A pushed cm is a lower bound rounded down to 64 or the previous cut + 64,
  // the previous cut being 0 or a pushed cm; it is above the previous cut and below m.)  The
  // schedule below and the strict launches' verdict words rely on it.
  return cuts;
}

// Vote slots of a call over `total` bytes in nch chunks: a vote list is allocated only when wholly
// inside its message (>= 72 B per vote), + the 64-slot alignment of each chunk of a chunked call.
// Slot indices travel as uint32: 0 = too many vote slots for one call.
inline uint64_t vote_slots(uint64_t total, size_t nch) {
  const uint64_t vt = total / 72 + 1 + (nch > 1 ? 64 * (uint64_t)nch : 0);
  return vt > 0xFFFFFFFFull ? 0 : vt;
}

// An arena's fields one after another, each from a 256-byte boundary.
struct ArenaWalk {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t at = off;
    off += align256(bytes);
    return at;
  }
};

// The call arena of a host call (byte offsets): the staged message bytes with 16 bytes of readable
// padding, their offsets, and the codes, records and digests on their way back.  What
// nwc_sanitize_messages_ex adds lies behind them, so a call without it keeps the layout above:
// with own_state the per-message gc_rounds (u64) and vote targets (80 B, SanGroupBuf's record), with
// votes the Vote::new signatures (64 B) and the "voted" bytes on their way back; with views
// (nwc_sanitize_messages_view) the view records (MSG_VIEW_BYTES each), the body of
// view_body_bound(total, m) bytes and the body allocator's counter, behind all of those.
struct CallArena {
  size_t data, offsets, codes, rec, digests;
  size_t gc_rounds, targets;      // own_state only
  size_t vote_sigs, voted;        // votes only
  size_t views, body, body_used;  // views only
  size_t bytes;
};
constexpr size_t MSG_TARGET_STRIDE = 80;
constexpr size_t MSG_VIEW_BYTES = 160;
// What the body of a view call can hold at most: per message 36 P + 32 Q + 8 V bytes in three
// 16-byte-aligned areas (<= 45 bytes of alignment), less than its wire length + 64 (a header's fixed
// fields alone take more than 160 bytes, a payload entry 36, a parent 32 and a vote >= 72).
constexpr uint64_t SAN_VIEW_SLACK = 64;   // per message, on top of its wire length
inline uint64_t view_body_bound(uint64_t total, uint64_t m) { return total + SAN_VIEW_SLACK * m; }
inline CallArena call_arena(size_t m, uint64_t total, bool own_state = false, bool votes = false, bool views = false) {
  ArenaWalk w;
  CallArena a{};
  a.data = w.take(total + 16);
  a.offsets = w.take(8 * (m + 1));
  a.codes = w.take(4 * m);
  a.rec = w.take(16 * m);
  a.digests = w.take(32 * m);   // (reserved whether or not the caller asks for digests)
  if (own_state) {
    a.gc_rounds = w.take(8 * m);
    a.targets = w.take(MSG_TARGET_STRIDE * m);
  }
  if (votes) {
    a.vote_sigs = w.take(64 * m);
    a.voted = w.take(m);
  }
  if (views) {
    a.views = w.take(MSG_VIEW_BYTES * m);
    a.body = w.take(view_body_bound(total, m));
    a.body_used = w.take(8);
  }
  a.bytes = w.off;
  return a;
}

// The message arena (byte offsets): the whole call's per-message and per-vote arrays (MsgArgs), the
// strict and leaf verdict words, and with ysplit the SignRecs of the votes (sr_*, vote v at index
// v) and of the strict equations (srs_*, message i at index i).
struct MsgArena {
  size_t hashbuf, eq_msg, eq_pk, eq_sig, cdig, v_pk, v_sig, v_msg, v_total, hmatch, rec, rec_n, sbits, lbits;
  size_t sr_x, sr_z, sr_p, sr_meta, srs_x, srs_z, srs_p, srs_meta;   // ysplit only
  size_t digests;                                                    // own_digests only
  size_t bytes;
};
// own_rec: the records live here (a caller that supplies its own array leaves `rec` unused: the
// fields after it move up, and its bytes are still counted).  own_digests: a call that signs votes
// while its caller takes no digests keeps them here, behind everything else.
inline MsgArena msg_arena(size_t m, uint64_t total, uint64_t vt, bool ysplit, bool own_rec, bool own_digests = false) {
  ArenaWalk w;
  MsgArena a{};
  a.hashbuf = w.take(total + 128 * (m + 2));
  a.eq_msg = w.take(32 * m);
  a.eq_pk = w.take(32 * m);
  a.eq_sig = w.take(64 * m);
  a.cdig = w.take(32 * m);
  a.v_pk = w.take(32 * vt);
  a.v_sig = w.take(64 * vt);
  a.v_msg = w.take(4 * vt);
  a.v_total = w.take(4);
  a.hmatch = w.take(4 * m);
  if (own_rec) a.rec = w.take(16 * m);
  a.rec_n = w.take(4 * m);
  a.sbits = w.take(8 * ((m + 63) / 64));
  a.lbits = w.take(8 * ((vt + 63) / 64));
  if (ysplit) {
    a.sr_x = w.take(32 * vt);
    a.sr_z = w.take(32 * vt);
    a.sr_p = w.take(32 * vt);
    a.sr_meta = w.take(4 * vt);
    a.srs_x = w.take(32 * m);
    a.srs_z = w.take(32 * m);
    a.srs_p = w.take(32 * m);
    a.srs_meta = w.take(4 * m);
  }
  if (own_digests) a.digests = w.take(32 * m);
  a.bytes = w.off + (own_rec ? 0 : align256(16 * m));
  return a;
}

// A sanitizer handle's buffers (sanitizer_handle.h; byte offsets), for groups of up to max_msgs
// messages in byte_cap wire bytes.  The group's equations share one index space of
// entries = max_msgs + vote_slots(byte_cap, 1): message i's strict equation at i, vote slot v at
// max_msgs + v.
//   SanGroupBuf: one pinned group buffer -- the wire bytes with 16 bytes of readable padding, the
//     per-message starts, lengths, gc_rounds and vote targets (80 B), and on the way back the result
//     words, digests and kinds; then what a vote request adds (nwc_sanitizer_sanitize_vote): the
//     device address of the signer's key record (8 B, 0 = no vote asked), the vote's signature
//     (64 B) and its "written" byte; then what a view request adds (nwc_sanitizer_sanitize_view):
//     the "view wanted" byte, the 160-byte record, the body bytes it used (u32) and the view's
//     "written" byte per message, and the group's body area of byte_cap + 64 max_msgs bytes, of
//     which message i owns [starts[i] + 64 i, starts[i] + lens[i] + 64 (i + 1)).
//   SanScratch: the HBM scratch of the handle (one group runs at a time on the device's stream).
//     eq_msg is followed by cdig (one digest array of 2 x max_msgs); `counters` is the vote-slot
//     allocator and the list count.
struct SanGroupBuf {
  size_t data, starts, lens, gc_rounds, targets, results, digests, kinds, vote_keys, vote_sigs, vote_flags;
  size_t view_wanted, views, view_used, view_flags, view_body;
  size_t bytes;
};
inline SanGroupBuf san_group_buf(size_t max_msgs, uint64_t byte_cap) {
  ArenaWalk w;
  SanGroupBuf a;
  a.data = w.take(byte_cap + 16);
  a.starts = w.take(8 * max_msgs);
  a.lens = w.take(4 * max_msgs);
  a.gc_rounds = w.take(8 * max_msgs);
  a.targets = w.take(80 * max_msgs);
  a.results = w.take(4 * max_msgs);
  a.digests = w.take(32 * max_msgs);
  a.kinds = w.take(max_msgs);
  a.vote_keys = w.take(8 * max_msgs);
  a.vote_sigs = w.take(64 * max_msgs);
  a.vote_flags = w.take(max_msgs);
  a.view_wanted = w.take(max_msgs);
  a.views = w.take(MSG_VIEW_BYTES * max_msgs);
  a.view_used = w.take(4 * max_msgs);
  a.view_flags = w.take(max_msgs);
  a.view_body = w.take(byte_cap + SAN_VIEW_SLACK * max_msgs);
  a.bytes = w.off;
  return a;
}
struct SanScratch {
  size_t hashbuf, eq_msg, eq_pk, eq_sig, msg_index, modes, vbytes, list, counters, hmatch, rec, rec_n, digests;
  uint64_t vote_slots, entries;
  size_t bytes;
};
inline SanScratch san_scratch(size_t max_msgs, uint64_t byte_cap) {
  ArenaWalk w;
  SanScratch a{};
  a.vote_slots = vote_slots(byte_cap, 1);
  a.entries = max_msgs + a.vote_slots;
  a.hashbuf = w.take(byte_cap + 128 * (max_msgs + 2));
  a.eq_msg = w.take(64 * max_msgs);
  a.eq_pk = w.take(32 * a.entries);
  a.eq_sig = w.take(64 * a.entries);
  a.msg_index = w.take(4 * a.entries);
  a.modes = w.take(a.entries);
  a.vbytes = w.take(a.entries);
  a.list = w.take(4 * a.entries);
  a.counters = w.take(8);
  a.hmatch = w.take(4 * max_msgs);
  a.rec = w.take(16 * max_msgs);
  a.rec_n = w.take(4 * max_msgs);
  a.digests = w.take(32 * max_msgs);
  a.bytes = w.off;
  return a;
}

// The pinned stage as the message pipeline uses it: the chunks' vote counts (uint32 each, read
// back asynchronously) in the first 64 KiB, the host call's message offsets above them.
constexpr size_t STAGE_COUNTS_AT = 0, STAGE_COUNTS_BYTES = 64u << 10;
constexpr size_t STAGE_OFFSETS_AT = STAGE_COUNTS_AT + STAGE_COUNTS_BYTES;
constexpr size_t stage_chunk_limit() { return STAGE_COUNTS_BYTES / sizeof(uint32_t); }
// whether m messages' offsets fit beside the counts in a stage of stage_max bytes
inline bool stage_holds_offsets(size_t m, size_t stage_max) { return 8 * (m + 1) <= stage_max - STAGE_OFFSETS_AT; }

// What a call of nch chunks defers and where its early strict launch goes.
struct MsgSchedule {
  bool chunked;    // more than one chunk: the leaves on the side stream beside the next chunk's parse
  // the leaf launches of a chunked call on the committee-cache comb path only list their uncached
  // equations (LV_DEFER_LIST); the list's half-size, fallback and torsion passes run once, after
  // the leaves queued before the first strict launch (which reuses the list), instead of ~8 small
  // launches per chunk on the leaf stream
  bool defer;
  // ... and their sign tests are deferred too (SignRecs, k_verify_comb_y / k_comb_sign): a chunk's
  // ~1 vote per lane would otherwise pay a whole inversion per vote.  NWC_SIGN_DEFER=0:
  // k_verify_comb per chunk (A/B).
  bool ysplit;
  // With the cache holding exactly the configured committee (cm_is_config) and the sign tests
  // deferred, the strict equations go on the parse stream as k_verify_comb_y without a list (an
  // uncached key is a non-member: UnknownAuthority decides first) and their sign pass, off the
  // leaf stream, which then carries only the leaves and their list passes.  NWC_STRICT_Y=0: through
  // launch_verify on the leaf stream (A/B).
  bool strict_y;
  // The strict equations of chunks [0, strict_at] go in one launch after chunk strict_at's leaves,
  // early, where the leaf stream has slack to absorb its ~0.17 ms (a latency-bound launch); the
  // rest at the end (every interior cut is a multiple of 64 messages, message_cuts: each strict
  // launch owns its verdict words).  (A strict launch per chunk, each after a list pass, measured
  // 20 % slower; at chunk nch - 3 instead of nch / 3, within noise: profiles/r06/wire_sign/.)
  size_t strict_at;
};
// deferrable: launch_verify takes the committee-cache comb path for any n (deferrable_list)
inline MsgSchedule schedule(size_t nch, bool deferrable, bool cm_is_config, const Settings& st) {
  MsgSchedule p;
  p.chunked = nch > 1;
  p.defer = p.chunked && deferrable;
  p.ysplit = p.defer && st.sign_defer;
  p.strict_y = p.ysplit && cm_is_config && st.strict_y;
  p.strict_at = nch >= 3 ? nch / 3 : 0;
  return p;
}

}  // namespace plan
}  // namespace nwc
