// Group formation for concurrent small verify calls (nwc_verifier, verifier.h): blocking requests
// from many threads are packed into shared launches.  No HIP in here -- the queue drives a Backend
// ("launch this group", "is this byte range done", "decide these equations again"), so that it
// runs against a fake backend under the host sanitizers (tests/cpp/verify_queue_host.cpp).
//
// A group is the set of requests that share a launch.  It lives in one of the backend's group
// buffers: a request reserves a range of equations in the open group under the queue lock and
// copies its inputs there outside it.  The thread that opened the group is its leader: it waits for
// the group to close, for the members' copies to finish, and launches; every member then polls its
// own verdict bytes (bit 7 written, bit 0 valid, bit 1 "decide me again") and leaves as soon as
// they are in.  The buffer is free again when the last member has left.
//
// A group closes when it holds max_requests requests, when the next request's equations do not
// fit, when max_wait_us have passed since it was opened, or -- max_wait_us == 0 -- as soon as no
// earlier group is in flight: a lone caller launches at once, and under load a group is whatever
// arrived while the previous one was busy.
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "nwc.h"

namespace nwc {
namespace vq {

// Host pointers into one group buffer of `cap` equations and `max_requests` requests.
struct GroupBuf {
  uint8_t* digests = nullptr;     // 32 B per request
  uint32_t* msg_index = nullptr;  // per equation: the request whose digest it checks
  uint8_t* pks = nullptr;         // 32 B per equation
  uint8_t* sigs = nullptr;        // 64 B per equation
  uint8_t* modes = nullptr;       // per equation, bit 0 = strict
  uint32_t* lists = nullptr;      // 2 x cap: the backend's equation lists (cached, first sight)
  uint8_t* vbytes = nullptr;      // per equation: the verdict byte
};

struct Backend {
  virtual ~Backend() = default;
  virtual GroupBuf buffer(int b) = 0;
  // Enqueue the work that decides equations [0, neq) of buffer b (nreq requests) and return without
  // waiting for it; wide / cold: how many equations went to each kernel.  0, or an error < 0 that
  // every member of the group receives.
  virtual int launch(int b, uint32_t nreq, uint32_t neq, uint32_t& wide, uint32_t& cold) = 0;
  // Every verdict byte of [lo, lo + n) written?
  virtual bool range_done(int b, uint32_t lo, uint32_t n) {
    const uint8_t* vb = buffer(b).vbytes;
    for (uint32_t i = 0; i < n; ++i)
      if (!(__atomic_load_n(vb + lo + i, __ATOMIC_ACQUIRE) & 0x80u)) return false;
    return true;
  }
  // Wait for everything launched for buffer b (a member's poll timed out): 0, or the error < 0.
  virtual int wait(int b) = 0;
  // Decide equations idx[0 .. m) of buffer b again, all of one mode: out[j] = 1 valid, 0 invalid.
  virtual int redo(int b, const uint32_t* idx, uint32_t m, bool strict, uint8_t* out) = 0;
  // A request too large for a group, decided outside the queue.
  virtual int bypass(const uint8_t* msg32, const uint8_t* pks, const uint8_t* sigs, size_t n, bool strict,
                     uint8_t* valid) = 0;
  // Called by a group's leader once it has its own results and has left the group.
  virtual void settle() {}
};

struct Stats {
  uint64_t groups = 0, requests = 0, equations = 0, wide_equations = 0, cold_equations = 0, redone_equations = 0,
           bypassed_requests = 0, max_requests_in_group = 0;
};

class Queue {
 public:
  using clock = std::chrono::steady_clock;

  // nbuf >= 2 group buffers of eq_cap equations; a request of more than req_max equations is
  // bypassed; poll_timeout: how long a member polls before it asks the backend to wait.
  Queue(Backend& be, uint32_t nbuf, uint32_t max_requests, uint32_t eq_cap, uint32_t req_max, uint32_t max_wait_us,
        std::chrono::microseconds poll_timeout = std::chrono::milliseconds(200))
      : be_(be), groups_(nbuf < 2 ? 2 : nbuf), max_req_(max_requests == 0 || max_requests > eq_cap ? eq_cap : max_requests),
        cap_(eq_cap), req_max_(req_max < eq_cap ? req_max : eq_cap), max_wait_(max_wait_us), poll_timeout_(poll_timeout) {}

  uint32_t max_requests() const { return max_req_; }
  uint32_t capacity() const { return cap_; }

  // One request: n equations over the digest msg32, all strict or all batch leaves.  valid[i] = 1
  // or 0.  Returns 0, or an error < 0 (the group's launch failed, the device reported an error, or
  // the queue was stopped: NWC_ERR_NOT_INIT).
  int submit(const uint8_t* msg32, const uint8_t* pks, const uint8_t* sigs, size_t n, bool strict, uint8_t* valid) {
    if (n == 0) return 0;
    std::unique_lock<std::mutex> lk(mu_);
    if (stopping_) return NWC_ERR_NOT_INIT;
    ++users_;
    int rc;
    if (n > req_max_) {
      ++stats_.bypassed_requests;
      lk.unlock();
      rc = be_.bypass(msg32, pks, sigs, n, strict, valid);
      lk.lock();
    } else {
      rc = grouped(lk, msg32, pks, sigs, (uint32_t)n, strict, valid);
    }
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
  struct Group {
    State state = FREE;
    uint32_t nreq = 0, neq = 0;
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
  // one step of a spin: a pause, and every 256th step the processor to whoever waits for it (with
  // as many spinning callers as processors, the thread they wait for needs one too)
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

  int grouped(std::unique_lock<std::mutex>& lk, const uint8_t* msg32, const uint8_t* pks, const uint8_t* sigs, uint32_t n,
              bool strict, uint8_t* valid) {
    // a place in the open group, or a free buffer to open the next one in
    int b = -1;
    bool leader = false;
    for (;;) {
      if (open_ >= 0) {
        Group& o = groups_[open_];
        if (o.nreq < max_req_ && o.neq + n <= cap_) { b = open_; break; }
        close(o);   // full, or this request does not fit: its leader launches it
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
    const uint32_t lo = g.neq, req = g.nreq;
    g.neq += n;
    ++g.nreq;
    ++g.refs;
    ++g.copying;
    ++stats_.requests;        // counted on arrival: a caller can see who is already waiting in a group
    stats_.equations += n;
    if (g.nreq == max_req_ || g.neq == cap_) close(g);
    lk.unlock();
    const GroupBuf gb = be_.buffer(b);
    std::memcpy(gb.digests + 32 * (size_t)req, msg32, 32);
    for (uint32_t i = 0; i < n; ++i) gb.msg_index[lo + i] = req;
    std::memcpy(gb.pks + 32 * (size_t)lo, pks, 32 * (size_t)n);
    std::memcpy(gb.sigs + 64 * (size_t)lo, sigs, 64 * (size_t)n);
    std::memset(gb.modes + lo, strict ? 1 : 0, n);
    for (uint32_t i = 0; i < n; ++i) __atomic_store_n(gb.vbytes + lo + i, (uint8_t)0, __ATOMIC_RELAXED);
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
      const uint32_t nreq = g.nreq, neq = g.neq;
      lk.unlock();
      uint32_t wide = 0, cold = 0;
      const int lrc = be_.launch(b, nreq, neq, wide, cold);
      lk.lock();
      g.t_launch = clock::now();
      g.rc = lrc;
      g.state = lrc ? FAILED : LAUNCHED;
      ++stats_.groups;
      stats_.wide_equations += wide;
      stats_.cold_equations += cold;
      if (nreq > stats_.max_requests_in_group) stats_.max_requests_in_group = nreq;
      signal();
    } else {
      await(lk, [&] { return g.state == LAUNCHED || g.state == FAILED; });
    }

    int rc = g.state == FAILED ? g.rc : 0;
    uint32_t redone = 0;
    if (rc == 0) {
      const clock::time_point t0 = g.t_launch;
      lk.unlock();
      rc = collect(b, gb, lo, n, strict, t0, valid, redone);
      lk.lock();
    }
    stats_.redone_equations += redone;
    if (--g.refs == 0) {
      g.state = FREE;
      signal();
    }
    if (leader) {
      lk.unlock();
      be_.settle();
      lk.lock();
    }
    return rc;
  }
  // an earlier group is closed or in flight and its members have not all left
  bool busy_other(const Group& g) const {
    for (const Group& o : groups_)
      if (&o != &g && o.state != FREE && o.state != OPEN) return true;
    return false;
  }

  // a member's own results: poll its bytes, fall back to the backend's wait, redo what asks for it
  int collect(int b, const GroupBuf& gb, uint32_t lo, uint32_t n, bool strict, clock::time_point t0, uint8_t* valid,
              uint32_t& redone) {
    for (uint32_t spins = 0; !be_.range_done(b, lo, n); ++spins) {
      if ((spins & 255) == 255 && clock::now() - t0 > poll_timeout_) {
        if (int rc = be_.wait(b)) return rc;
        break;
      }
      relax(spins);
    }
    std::vector<uint32_t> again;
    for (uint32_t i = 0; i < n; ++i) {
      const uint8_t v = __atomic_load_n(gb.vbytes + lo + i, __ATOMIC_ACQUIRE);
      if (!(v & 0x80u) || (v & 2u)) again.push_back(lo + i);   // unwritten after the wait, or "decide me again"
      else valid[i] = v & 1u;
    }
    if (again.empty()) return 0;
    std::vector<uint8_t> out(again.size(), 0);
    if (int rc = be_.redo(b, again.data(), (uint32_t)again.size(), strict, out.data())) return rc;
    for (size_t j = 0; j < again.size(); ++j) valid[again[j] - lo] = out[j] & 1u;
    redone = (uint32_t)again.size();
    return 0;
  }

  Backend& be_;
  std::vector<Group> groups_;
  const uint32_t max_req_, cap_, req_max_, max_wait_;
  const std::chrono::microseconds poll_timeout_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::atomic<uint64_t> epoch_{0};
  int open_ = -1;
  uint32_t users_ = 0;
  bool stopping_ = false;
  Stats stats_;
};

}  // namespace vq
}  // namespace nwc
