// Group formation for concurrent one-message sanitize calls (nwc_sanitizer, sanitizer_handle.h):
// blocking requests from many threads, each carrying one wire message, are packed into shared
// pipeline launches.  No HIP in here -- like verify_queue.h, the queue drives a Backend ("launch
// this group", "wait for it", "decide this message again"), so that it runs against a fake backend
// under the host sanitizers (tests/cpp/sanitize_queue_host.cpp).
//
// A group is the set of requests that share one set of launches.  It lives in one of the backend's
// group buffers: a request reserves a message slot and a byte range in the open group under the
// queue lock -- the range starts 16-byte aligned, as a digester arena batch does -- and outside the
// lock copies its bytes, its gc_round and its vote target there and clears its result word.  The
// thread that opened the group is its leader: it waits for the group to close, for the members'
// copies to finish, and launches; every member then polls its own result word (bit 31 written, bit
// 30 "decide me again", bits 8-23 the equations the message listed, bits 0-7 the code) and leaves
// as soon as it is in.  The buffer is free again when the last member has left.
//
// A group closes when it holds max_messages messages, when the next message's bytes do not fit,
// when max_wait_us have passed since it was opened, or -- max_wait_us == 0 -- as soon as no earlier
// group is in flight: a lone caller launches at once, and under load a group is whatever arrived
// while the previous one was busy.
//
// A request may ask for Vote::new on its header (submit's vote_key: the device address of a signer's
// key record).  Every member writes its slot's key -- 0 when it asks for none, so that a key left by
// the buffer's previous group is never signed for -- and clears its slot's vote flag byte; the
// backend's launch signs, inside the same flight, for the slots that carry a key and whose word
// says Ok + header.  Such a member polls its flag byte after its result word.  A vote the flight did
// not deliver (flag unwritten, message redone or bypassed) comes from Backend::vote_alone, asked
// only once the message's code is known to be Ok and its kind a header: never speculatively.
//
// A request may also ask for the device's decode of its message (submit's view: a 160-byte
// nwc_msg_view record plus a body).  The protocol is the vote's: every member writes its slot's
// "view wanted" byte, 0 included, and clears its view flag byte; the backend's launch builds the
// records of the slots that ask, each body in the slot's own region of the group's body area
// (view_region: no allocator, nothing to reset between groups).  Such a member polls its view flag
// after its result word and before its vote flag -- the backend queues the views before the votes,
// so a member that wants only the cheap one does not wait for a signature, and polling in stream
// order costs a member that wants both nothing: when the later flag is in the earlier one is.  A
// view the flight did not deliver comes from Backend::view_alone, which for a message that was
// redone or bypassed also DECIDES it (redo / bypass are then not called: one decision, not two).
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "nwc.h"

namespace nwc {
namespace sq {

constexpr uint32_t R_WRITTEN = 1u << 31, R_REDO = 1u << 30;
constexpr size_t TARGET_STRIDE = 80;   // id(32) round(8, LE) origin(32), then the "enabled" byte
constexpr size_t TARGET_FLAG_AT = 72;
constexpr uint64_t RANGE_ALIGN = 16;

inline uint64_t align_range(uint64_t x) { return (x + (RANGE_ALIGN - 1)) & ~(RANGE_ALIGN - 1); }
inline uint32_t result_code(uint32_t w) { return w & 255u; }
inline uint32_t result_equations(uint32_t w) { return (w >> 8) & 0xFFFFu; }

// Host pointers into one group buffer of `byte_cap` wire bytes and `max_messages` messages.
struct GroupBuf {
  uint8_t* data = nullptr;        // wire bytes; at least 16 readable bytes follow byte_cap
  uint64_t* starts = nullptr;     // per message: where its bytes begin in data (16-byte aligned)
  uint32_t* lens = nullptr;       // per message: its length
  uint64_t* gc_rounds = nullptr;  // per message
  uint8_t* targets = nullptr;     // per message, TARGET_STRIDE bytes
  uint32_t* results = nullptr;    // per message: the result word
  uint8_t* digests = nullptr;     // per message, 32 B: written before the result word
  uint8_t* kinds = nullptr;       // per message: written before the result word
  uint64_t* vote_keys = nullptr;  // per message: the vote request's key (0 = none); null: a backend without votes
  uint8_t* vote_sigs = nullptr;   // per message, 64 B: written before the vote flag
  uint8_t* vote_flags = nullptr;  // per message: bit 7 = the vote's signature is in
  uint8_t* view_wanted = nullptr; // per message: non-zero = a view is asked for; null: a backend without views
  uint8_t* views = nullptr;       // per message, VIEW_BYTES: written before the view flag
  uint32_t* view_used = nullptr;  // per message: the body bytes the view took, written before the view flag
  uint8_t* view_flags = nullptr;  // per message: bit 7 = the record, its body and view_used are in
  uint8_t* view_body = nullptr;   // the group's body area: byte_cap + VIEW_SLACK * max_messages bytes
};

constexpr uint8_t VOTE_WRITTEN = 0x80;
constexpr uint8_t VIEW_WRITTEN = 0x80;
constexpr size_t VIEW_BYTES = 160;    // one nwc_msg_view
constexpr uint64_t VIEW_SLACK = 64;   // a message's body holds at most its length + VIEW_SLACK bytes
inline uint64_t view_body_bound(uint64_t len) { return len + VIEW_SLACK; }   // nwc_msg_view_body_bound(len, 1)
// where slot `slot` of a group, whose bytes start at `start` of the data, has its body region
inline uint64_t view_region(uint64_t start, uint32_t slot) { return start + VIEW_SLACK * slot; }

// A request's view outputs: the record (VIEW_BYTES), the body (cap >= view_body_bound(len)) and the
// body bytes in use.  All three are required.
struct ViewReq {
  uint8_t* rec = nullptr;
  uint8_t* body = nullptr;
  uint64_t body_cap = 0;
  uint64_t* body_used = nullptr;
};
constexpr uint32_t KIND_HEADER = 0;   // PrimaryMessage::Header, as the kinds array and the kind output carry it

struct Backend {
  virtual ~Backend() = default;
  virtual GroupBuf buffer(int b) = 0;
  // Enqueue the work that decides messages [0, nmsg) of buffer b (bytes [0, nbytes) of its data)
  // and return without waiting for it.  0, or an error < 0 that every member of the group receives.
  virtual int launch(int b, uint32_t nmsg, uint64_t nbytes) = 0;
  // Wait for everything launched for buffer b (a member's poll timed out): 0, or the error < 0.
  virtual int wait(int b) = 0;
  // Decide one message again, outside the group: the code >= 0, or an error < 0.
  virtual int redo(const uint8_t* msg, size_t len, uint64_t gc_round, const uint8_t* vote_target, uint8_t* digest32,
                   uint8_t* kind) = 0;
  // A message that does not go through a group (larger than one, or the caller asked): as redo.
  virtual int bypass(const uint8_t* msg, size_t len, uint64_t gc_round, const uint8_t* vote_target, uint8_t* digest32,
                     uint8_t* kind) = 0;
  // Vote::new for one message that was decided Ok and is a header (id32: its digest), outside a
  // group: 0 and the signature under vote_key in sig64, or an error < 0.  A backend without votes
  // keeps this default.
  virtual int vote_alone(const uint8_t* /*msg*/, size_t /*len*/, const uint8_t* /*id32*/, uint64_t /*vote_key*/,
                         uint8_t* /*sig64*/) {
    return NWC_ERR_ARG;
  }
  // Decide one message outside a group AND hand back its view: the code >= 0 with digest32, kind,
  // the record and the body filled (*body_used bytes of it), or an error < 0.  A backend without
  // views keeps this default.
  virtual int view_alone(const uint8_t* /*msg*/, size_t /*len*/, uint64_t /*gc_round*/, const uint8_t* /*vote_target*/,
                         uint8_t* /*digest32*/, uint8_t* /*kind*/, const ViewReq& /*out*/) {
    return NWC_ERR_ARG;
  }
};

struct Stats {
  uint64_t groups = 0, messages = 0, bytes = 0, equations = 0, redone_messages = 0, bypassed_messages = 0,
           max_messages_in_group = 0, reserved = 0;
  uint64_t votes_in_flight = 0, votes_alone = 0;   // votes signed inside a group flight / by vote_alone
  uint64_t views_in_flight = 0, views_alone = 0;   // views built inside a group flight / by view_alone
};

class Queue {
 public:
  using clock = std::chrono::steady_clock;

  // nbuf >= 2 group buffers of byte_cap bytes and msg_cap messages; a group closes at max_messages
  // (0 or more than msg_cap: msg_cap); poll_timeout: how long a member polls before it asks the
  // backend to wait.
  Queue(Backend& be, uint32_t nbuf, uint32_t max_messages, uint32_t msg_cap, uint64_t byte_cap, uint32_t max_wait_us,
        std::chrono::microseconds poll_timeout = std::chrono::milliseconds(200))
      : be_(be), groups_(nbuf < 2 ? 2 : nbuf), max_msg_(max_messages == 0 || max_messages > msg_cap ? msg_cap : max_messages),
        byte_cap_(byte_cap), max_wait_(max_wait_us), poll_timeout_(poll_timeout) {}

  uint32_t max_messages() const { return max_msg_; }
  uint64_t byte_capacity() const { return byte_cap_; }

  // One request: one wire message under its own gc_round and vote target (72 bytes or nullptr).
  // Returns the message's code >= 0 (digest32 and kind, both nullable, filled), or an error < 0
  // (the group's launch failed, the device reported an error, or the queue was stopped:
  // NWC_ERR_NOT_INIT).  direct: hand the message to Backend::bypass whatever its size.
  // vote_key != 0 asks for Vote::new under that key when the message is a header and its code is
  // Ok: vote_sig (64 bytes) then holds the signature and *voted is 1; otherwise -- an error
  // included -- *voted is 0 and vote_sig is zeroed.  Both are required with a key.
  // view != nullptr asks for the message's view: its three outputs are required and body_cap >=
  // view_body_bound(len), else NWC_ERR_ARG before anything is queued.  On an error < 0 the record is
  // zeroed and *body_used is 0.
  int submit(const uint8_t* msg, size_t len, uint64_t gc_round, const uint8_t* vote_target, uint8_t* digest32, uint8_t* kind,
             bool direct = false, uint64_t vote_key = 0, uint8_t* vote_sig = nullptr, int* voted = nullptr,
             const ViewReq* view = nullptr) {
    if (vote_sig) std::memset(vote_sig, 0, 64);
    if (voted) *voted = 0;
    View vw;
    if (view) {
      vw.out = *view;
      vw.asked = true;
      if (vw.out.rec) std::memset(vw.out.rec, 0, VIEW_BYTES);
      if (vw.out.body_used) *vw.out.body_used = 0;
      if (!vw.out.rec || !vw.out.body || !vw.out.body_used || vw.out.body_cap < view_body_bound(len)) return NWC_ERR_ARG;
    }
    if (vote_key && (!vote_sig || !voted)) return NWC_ERR_ARG;
    std::unique_lock<std::mutex> lk(mu_);
    if (stopping_) return NWC_ERR_NOT_INIT;
    ++users_;
    int rc;
    Vote v{vote_key, vote_sig, voted};
    if (direct || len > byte_cap_) {
      ++stats_.bypassed_messages;
      lk.unlock();
      // (the vote needs the digest and the kind whether or not the caller asked for them)
      uint8_t dig[32], kd = 0xFF;
      rc = outside(false, msg, len, gc_round, vote_target, vote_key ? dig : digest32, vote_key ? &kd : kind, vw);
      if (vote_key && rc >= 0 && (rc = vote_outside(msg, len, rc, dig, kd, v)) >= 0) {   // (an error touches no output)
        if (digest32) std::memcpy(digest32, dig, 32);
        if (kind) *kind = kd;
      }
      lk.lock();
    } else {
      rc = grouped(lk, msg, len, gc_round, vote_target, digest32, kind, v, vw);
    }
    if (rc < 0 && vw.asked) {
      std::memset(vw.out.rec, 0, VIEW_BYTES);
      *vw.out.body_used = 0;
      vw.in_flight = vw.alone = false;
    }
    stats_.votes_in_flight += v.in_flight ? 1 : 0;
    stats_.votes_alone += v.alone ? 1 : 0;
    stats_.views_in_flight += vw.in_flight ? 1 : 0;
    stats_.views_alone += vw.alone ? 1 : 0;
    if (--users_ == 0) signal();
    return rc;
  }

  // destroy / shutdown: open groups close at once, queued requests finish, later ones are refused;
  // returns when every caller has left.
  void stop() {
    std::unique_lock<std::mutex> lk(mu_);
    stopping_ = true;
    signal();
    await(lk, [&] { return users_ == 0; });
  }

  Stats stats() {
    std::lock_guard<std::mutex> lk(mu_);
    return stats_;
  }

 private:
  enum State { FREE, OPEN, CLOSED, LAUNCHED, FAILED };
  // one request's vote: what it asked for and which route delivered it
  struct Vote {
    uint64_t key;
    uint8_t* sig;
    int* voted;
    bool in_flight = false, alone = false;
  };
  // one request's view: where it goes and which route delivered it
  struct View {
    ViewReq out;
    bool asked = false, in_flight = false, alone = false;
  };
  // a message decided outside a group: by redo / bypass, or -- a view request -- by view_alone, which
  // decides it and builds its view in one call.  Returns the code, or the backend's error.
  int outside(bool again, const uint8_t* msg, size_t len, uint64_t gc_round, const uint8_t* vote_target, uint8_t* digest32,
              uint8_t* kind, View& vw) {
    if (!vw.asked)
      return again ? be_.redo(msg, len, gc_round, vote_target, digest32, kind)
                   : be_.bypass(msg, len, gc_round, vote_target, digest32, kind);
    const int rc = be_.view_alone(msg, len, gc_round, vote_target, digest32, kind, vw.out);
    if (rc >= 0 && *vw.out.body_used > vw.out.body_cap) return NWC_ERR_DEVICE;
    vw.alone = rc >= 0;
    return rc;
  }
  // a message decided outside a group (redo, bypass) or whose flag stayed unwritten: the vote comes
  // from the backend, and only for an Ok header.  Returns the code, or vote_alone's error.
  int vote_outside(const uint8_t* msg, size_t len, int code, const uint8_t* id32, uint8_t kind, Vote& v) {
    if (!v.key || code != 0 || kind != KIND_HEADER) return code;
    if (int rc = be_.vote_alone(msg, len, id32, v.key, v.sig)) {
      std::memset(v.sig, 0, 64);
      return rc < 0 ? rc : NWC_ERR_DEVICE;
    }
    *v.voted = 1;
    v.alone = true;
    return code;
  }
  struct Group {
    State state = FREE;
    uint32_t nmsg = 0;
    uint64_t nbytes = 0;    // end of the last reserved range
    uint32_t copying = 0;   // members still copying their inputs in
    uint32_t refs = 0;      // members that have not left
    int rc = 0;             // FAILED: what every member returns
    clock::time_point t_open, t_launch;
  };

  // every state change happens under mu_ and ends in signal(); a waiter spins on the epoch for a
  // short while (a group's flight time) before it sleeps on the condition variable
  void signal() {
    epoch_.fetch_add(1, std::memory_order_release);
    cv_.notify_all();
  }
  // one step of a spin: a pause, and every 256th step the processor to whoever waits for it
  static void relax(uint32_t k) {
    if ((k & 255) == 255) std::this_thread::yield();
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#endif
  }
  // returns false if `deadline` passed before the state changed
  bool nap(std::unique_lock<std::mutex>& lk, const clock::time_point* deadline) {
    const uint64_t e = epoch_.load(std::memory_order_relaxed);
    lk.unlock();
    bool changed = false;
    for (int k = 0; k < 4096 && !changed; ++k) {
      relax(k);
      changed = epoch_.load(std::memory_order_acquire) != e;
      if (deadline && (k & 63) == 63 && clock::now() >= *deadline) break;
    }
    lk.lock();
    auto moved = [&] { return epoch_.load(std::memory_order_relaxed) != e; };
    if (moved()) return true;
    if (!deadline) {
      cv_.wait(lk, moved);
      return true;
    }
    // (a timed wait on the system clock: pthread_cond_timedwait, which every thread sanitizer
    // runtime knows; a jump of that clock only cuts this nap short or lets the next one end it)
    const auto left = *deadline - clock::now();
    if (left <= clock::duration::zero()) return false;
    return cv_.wait_until(lk, std::chrono::system_clock::now() + left, moved);
  }
  template <class P>
  void await(std::unique_lock<std::mutex>& lk, P pred) {
    while (!pred()) nap(lk, nullptr);
  }

  void close(Group& g) {
    g.state = CLOSED;
    open_ = -1;
    signal();
  }

  int grouped(std::unique_lock<std::mutex>& lk, const uint8_t* msg, size_t len, uint64_t gc_round, const uint8_t* vote_target,
              uint8_t* digest32, uint8_t* kind, Vote& v, View& vw) {
    // a place in the open group, or a free buffer to open the next one in
    int b = -1;
    bool leader = false;
    for (;;) {
      if (open_ >= 0) {
        Group& o = groups_[open_];
        if (o.nmsg < max_msg_ && align_range(o.nbytes) + len <= byte_cap_) { b = open_; break; }
        close(o);   // full, or this message does not fit: its leader launches it
      }
      for (size_t k = 0; k < groups_.size() && b < 0; ++k)
        if (groups_[k].state == FREE) b = (int)k;
      if (b >= 0) {
        Group& f = groups_[b];
        f = Group{};
        f.state = OPEN;
        f.t_open = clock::now();
        open_ = b;
        leader = true;
        break;
      }
      nap(lk, nullptr);   // every buffer busy
    }
    Group& g = groups_[b];
    const uint64_t lo = align_range(g.nbytes);
    const uint32_t slot = g.nmsg;
    g.nbytes = lo + len;
    ++g.nmsg;
    ++g.refs;
    ++g.copying;
    ++stats_.messages;        // counted on arrival: a caller can see who is already waiting in a group
    stats_.bytes += len;
    if (g.nmsg == max_msg_) close(g);
    lk.unlock();
    const GroupBuf gb = be_.buffer(b);
    if (len) std::memcpy(gb.data + lo, msg, len);
    gb.starts[slot] = lo;
    gb.lens[slot] = (uint32_t)len;
    gb.gc_rounds[slot] = gc_round;
    uint8_t* t = gb.targets + TARGET_STRIDE * (size_t)slot;
    if (vote_target) std::memcpy(t, vote_target, TARGET_FLAG_AT);
    else std::memset(t, 0, TARGET_FLAG_AT);
    std::memset(t + TARGET_FLAG_AT, 0, TARGET_STRIDE - TARGET_FLAG_AT);
    t[TARGET_FLAG_AT] = vote_target ? 1 : 0;
    __atomic_store_n(gb.results + slot, 0u, __ATOMIC_RELAXED);
    if (gb.vote_keys) {
      // The previous group's vote launch may still be running when its last member has left (a
      // member that asked for nothing leaves with its result word).  It reads a slot's key and then
      // its result word, so the cleared word must be out before a new key is: a late block that
      // sees this key then finds no "written" bit and leaves.  (A key of 0 needs no such order.)
      __atomic_store_n(gb.vote_flags + slot, (uint8_t)0, __ATOMIC_RELAXED);
      if (v.key) __atomic_thread_fence(__ATOMIC_SEQ_CST);
      __atomic_store_n(gb.vote_keys + slot, v.key, __ATOMIC_RELEASE);   // 0 included: the previous group's key goes
    }
    if (gb.view_wanted) {
      // the same order for the view: flag and word cleared, a full fence, then a non-zero wanted
      // byte -- the view launch reads the byte first and the word second
      __atomic_store_n(gb.view_flags + slot, (uint8_t)0, __ATOMIC_RELAXED);
      if (vw.asked) __atomic_thread_fence(__ATOMIC_SEQ_CST);
      __atomic_store_n(gb.view_wanted + slot, (uint8_t)(vw.asked ? 1 : 0), __ATOMIC_RELEASE);   // 0 included
    }
    lk.lock();
    if (--g.copying == 0) signal();

    if (leader) {
      while (g.state == OPEN) {
        if (stopping_) {
          close(g);
        } else if (max_wait_ == 0) {
          if (!busy_other(g)) close(g);
          else nap(lk, nullptr);
        } else {
          const clock::time_point deadline = g.t_open + std::chrono::microseconds(max_wait_);
          if (clock::now() >= deadline) close(g);
          else nap(lk, &deadline);
        }
      }
      await(lk, [&] { return g.copying == 0; });
      const uint32_t nmsg = g.nmsg;
      const uint64_t nbytes = g.nbytes;
      lk.unlock();
      const int lrc = be_.launch(b, nmsg, nbytes);
      lk.lock();
      g.t_launch = clock::now();
      g.rc = lrc;
      g.state = lrc ? FAILED : LAUNCHED;
      ++stats_.groups;
      if (nmsg > stats_.max_messages_in_group) stats_.max_messages_in_group = nmsg;
      signal();
    } else {
      await(lk, [&] { return g.state == LAUNCHED || g.state == FAILED; });
    }

    int rc = g.state == FAILED ? g.rc : 0;
    bool redone = false;
    uint32_t equations = 0;
    if (rc == 0) {
      const clock::time_point t0 = g.t_launch;
      lk.unlock();
      rc = collect(b, gb, slot, msg, len, gc_round, vote_target, t0, digest32, kind, redone, equations, v, vw);
      lk.lock();
    }
    stats_.redone_messages += redone ? 1 : 0;
    stats_.equations += equations;
    if (--g.refs == 0) {
      g.state = FREE;
      signal();
    }
    return rc;
  }
  // an earlier group is closed or in flight and its members have not all left
  bool busy_other(const Group& g) const {
    for (const Group& o : groups_)
      if (&o != &g && o.state != FREE && o.state != OPEN) return true;
    return false;
  }

  // a member's own result: poll its word, fall back to the backend's wait, redo if it asks for it
  int collect(int b, const GroupBuf& gb, uint32_t slot, const uint8_t* msg, size_t len, uint64_t gc_round,
              const uint8_t* vote_target, clock::time_point t0, uint8_t* digest32, uint8_t* kind, bool& redone,
              uint32_t& equations, Vote& v, View& vw) {
    uint32_t w = 0;
    for (uint32_t spins = 0; !((w = __atomic_load_n(gb.results + slot, __ATOMIC_ACQUIRE)) & R_WRITTEN); ++spins) {
      if ((spins & 255) == 255 && clock::now() - t0 > poll_timeout_) {
        if (int rc = be_.wait(b)) return rc;
        w = __atomic_load_n(gb.results + slot, __ATOMIC_ACQUIRE);
        break;
      }
      relax(spins);
    }
    if (!(w & R_WRITTEN) || (w & R_REDO)) {   // unwritten after the wait, or "decide me again"
      redone = true;
      if (!v.key) return outside(true, msg, len, gc_round, vote_target, digest32, kind, vw);
      uint8_t dig[32], kd = 0xFF;
      int rc = outside(true, msg, len, gc_round, vote_target, dig, &kd, vw);
      if (rc < 0 || (rc = vote_outside(msg, len, rc, dig, kd, v)) < 0) return rc;
      if (digest32) std::memcpy(digest32, dig, 32);
      if (kind) *kind = kd;
      return rc;
    }
    equations = result_equations(w);
    const int code = (int)result_code(w);
    const uint8_t kd = gb.kinds[slot];
    if (vw.asked) {
      // the flight builds the views behind the result words and before the votes: poll the slot's
      // view flag first, under the same time limit
      bool in = false;
      if (gb.view_flags) {
        auto written = [&] { return (__atomic_load_n(gb.view_flags + slot, __ATOMIC_ACQUIRE) & VIEW_WRITTEN) != 0; };
        for (uint32_t spins = 0; !(in = written()); ++spins) {
          if ((spins & 255) == 255 && clock::now() - t0 > poll_timeout_) {
            if (int rc = be_.wait(b)) return rc;
            in = written();
            break;
          }
          relax(spins);
        }
      }
      if (in) {
        const uint32_t used = gb.view_used[slot];
        if (used > view_body_bound(len)) return NWC_ERR_DEVICE;   // (cap >= the bound was checked on entry)
        std::memcpy(vw.out.rec, gb.views + VIEW_BYTES * (size_t)slot, VIEW_BYTES);
        if (used) std::memcpy(vw.out.body, gb.view_body + view_region(gb.starts[slot], slot), used);
        *vw.out.body_used = used;
        vw.in_flight = true;
      } else {
        // the flight's code, digest and kind stand; the batch entry's record must agree with them
        uint8_t dig[32], k2 = 0xFF;
        const int rc = be_.view_alone(msg, len, gc_round, vote_target, dig, &k2, vw.out);
        if (rc < 0) return rc;
        if (rc != code || k2 != kd || *vw.out.body_used > vw.out.body_cap) return NWC_ERR_DEVICE;
        vw.alone = true;
      }
    }
    if (v.key && code == 0 && kd == KIND_HEADER) {
      // the flight signs after the result words: poll the slot's flag under the same time limit
      bool in = false;
      if (gb.vote_flags) {
        auto written = [&] { return (__atomic_load_n(gb.vote_flags + slot, __ATOMIC_ACQUIRE) & VOTE_WRITTEN) != 0; };
        for (uint32_t spins = 0; !(in = written()); ++spins) {
          if ((spins & 255) == 255 && clock::now() - t0 > poll_timeout_) {
            if (int rc = be_.wait(b)) return rc;
            in = written();
            break;
          }
          relax(spins);
        }
      }
      if (in) {
        std::memcpy(v.sig, gb.vote_sigs + 64 * (size_t)slot, 64);
        *v.voted = 1;
        v.in_flight = true;
      } else if (int rc = vote_outside(msg, len, code, gb.digests + 32 * (size_t)slot, kd, v); rc < 0) {
        return rc;
      }
    }
    if (digest32) std::memcpy(digest32, gb.digests + 32 * (size_t)slot, 32);
    if (kind) *kind = kd;
    return code;
  }

  Backend& be_;
  std::vector<Group> groups_;
  const uint32_t max_msg_;
  const uint64_t byte_cap_;
  const uint32_t max_wait_;
  const std::chrono::microseconds poll_timeout_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::atomic<uint64_t> epoch_{0};
  int open_ = -1;
  uint32_t users_ = 0;
  bool stopping_ = false;
  Stats stats_;
};

}  // namespace sq
}  // namespace nwc
