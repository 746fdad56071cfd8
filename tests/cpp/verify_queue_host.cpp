// Drives narwhal_amd/csrc/verify_queue.h against a fake backend, on the CPU.  Built twice by
// tests/test_verify_queue_host.py (thread sanitizer; address + undefined-behaviour sanitizers) and
// run as a child process.  Exit status 0 and a last line "ok" mean every check held.
//
// The fake device decides an equation by its signature's first byte: valid = sig[0] & 1.  Further
// bytes of the signature steer the fake and carry what it checks:
//   sig[1] & 1  the device answers "decide me again" (bit 1) -> the queue must call redo
//   sig[2] & 1  the device never writes the byte -> poll time-out, wait, then redo
//   sig[3]      the mode the request was submitted with (checked against the mode byte)
//   sig[4]      first byte of the request's digest (checked through msg_index)
// A device thread completes each launch after a random delay; one chosen launch fails.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

#include "verify_queue.h"

namespace {

using nwc::vq::GroupBuf;

std::atomic<uint64_t> g_failures{0};
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      g_failures.fetch_add(1);                                           \
    }                                                                    \
  } while (0)

struct FakeBackend : nwc::vq::Backend {
  static constexpr int NBUF = 2;
  const uint32_t cap, max_req;
  const long fail_group;   // index of the launch that fails (-1 = none)
  const int max_delay_us;
  struct Mem {
    std::vector<uint8_t> digests, pks, sigs, modes, vbytes;
    std::vector<uint32_t> msg_index, lists;
  } mem[NBUF];
  // the fake device: one thread, launches complete in order after a random delay
  struct Job { int b; uint32_t neq; };
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Job> jobs;
  bool busy[NBUF] = {false, false};
  bool quit = false;
  std::thread device;
  std::atomic<long> launches{0};
  std::atomic<uint64_t> failed_requests{0}, redo_calls{0}, redo_equations{0}, waits{0}, bypasses{0}, max_nreq{0}, max_neq{0};

  FakeBackend(uint32_t cap_, uint32_t max_req_, long fail_group_, int max_delay_us_)
      : cap(cap_), max_req(max_req_), fail_group(fail_group_), max_delay_us(max_delay_us_) {
    for (Mem& m : mem) {
      m.digests.resize(32 * (size_t)max_req);
      m.msg_index.resize(cap);
      m.pks.resize(32 * (size_t)cap);
      m.sigs.resize(64 * (size_t)cap);
      m.modes.resize(cap);
      m.lists.resize(2 * (size_t)cap);
      m.vbytes.resize(cap);
    }
    device = std::thread([this] { run(); });
  }
  ~FakeBackend() override {
    {
      std::lock_guard<std::mutex> lk(mu);
      quit = true;
    }
    cv.notify_all();
    device.join();
  }
  void run() {
    std::mt19937 rng(12345);
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [&] { return quit || !jobs.empty(); });
      if (jobs.empty()) return;
      const Job j = jobs.front();
      jobs.pop_front();
      lk.unlock();
      if (max_delay_us) std::this_thread::sleep_for(std::chrono::microseconds(rng() % (max_delay_us + 1)));
      Mem& m = mem[j.b];
      for (uint32_t e = 0; e < j.neq; ++e) {
        const uint8_t* sig = &m.sigs[64 * (size_t)e];
        CHECK(m.modes[e] == sig[3]);
        CHECK(m.msg_index[e] < max_req && m.digests[32 * (size_t)m.msg_index[e]] == sig[4]);
        CHECK(__atomic_load_n(&m.vbytes[e], __ATOMIC_RELAXED) == 0);   // the member zeroed its range
        if (sig[2] & 1) continue;   // left unwritten
        const uint8_t v = (sig[1] & 1) ? 0x82u : (uint8_t)(0x80u | (sig[0] & 1u));
        __atomic_store_n(&m.vbytes[e], v, __ATOMIC_RELEASE);
      }
      lk.lock();
      busy[j.b] = false;
      cv.notify_all();
    }
  }

  GroupBuf buffer(int b) override {
    Mem& m = mem[b];
    GroupBuf g;
    g.digests = m.digests.data(); g.msg_index = m.msg_index.data(); g.pks = m.pks.data(); g.sigs = m.sigs.data();
    g.modes = m.modes.data(); g.lists = m.lists.data(); g.vbytes = m.vbytes.data();
    return g;
  }
  int launch(int b, uint32_t nreq, uint32_t neq, uint32_t& wide, uint32_t& cold) override {
    CHECK(nreq >= 1 && nreq <= max_req);
    CHECK(neq >= nreq && neq <= cap);
    uint64_t prev = max_nreq.load();
    while (nreq > prev && !max_nreq.compare_exchange_weak(prev, nreq)) {}
    prev = max_neq.load();
    while (neq > prev && !max_neq.compare_exchange_weak(prev, neq)) {}
    const long k = launches.fetch_add(1);
    if (k == fail_group) {
      failed_requests.fetch_add(nreq);
      return NWC_ERR_DEVICE;
    }
    wide = neq;
    cold = 0;
    std::lock_guard<std::mutex> lk(mu);
    CHECK(!busy[b]);   // a buffer is launched again only after its members have all left
    busy[b] = true;
    jobs.push_back(Job{b, neq});
    cv.notify_all();
    return 0;
  }
  int wait(int b) override {
    waits.fetch_add(1);
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return !busy[b]; });
    return 0;
  }
  int redo(int b, const uint32_t* idx, uint32_t m, bool strict, uint8_t* out) override {
    redo_calls.fetch_add(1);
    redo_equations.fetch_add(m);
    Mem& mm = mem[b];
    for (uint32_t j = 0; j < m; ++j) {
      CHECK(idx[j] < cap);
      const uint8_t* sig = &mm.sigs[64 * (size_t)idx[j]];
      CHECK((sig[1] & 1) || (sig[2] & 1));   // only equations that asked for it, or were left unwritten
      CHECK(sig[3] == (strict ? 1 : 0));
      out[j] = sig[0] & 1u;
    }
    return 0;
  }
  int bypass(const uint8_t*, const uint8_t*, const uint8_t* sigs, size_t n, bool, uint8_t* valid) override {
    bypasses.fetch_add(1);
    for (size_t i = 0; i < n; ++i) valid[i] = sigs[64 * i] & 1u;
    return 0;
  }
};

struct Request {
  std::vector<uint8_t> msg, pks, sigs, expect;
  bool strict;
};
Request make_request(std::mt19937& rng, uint32_t n, int redo_one_in, int lost_one_in) {
  Request r;
  r.strict = rng() & 1;
  r.msg.assign(32, (uint8_t)rng());
  r.pks.resize(32 * (size_t)n);
  r.sigs.assign(64 * (size_t)n, 0);
  r.expect.resize(n);
  for (uint8_t& x : r.pks) x = (uint8_t)rng();
  for (uint32_t i = 0; i < n; ++i) {
    uint8_t* sig = &r.sigs[64 * (size_t)i];
    sig[0] = (uint8_t)rng();
    sig[1] = redo_one_in && rng() % redo_one_in == 0;
    sig[2] = lost_one_in && rng() % lost_one_in == 0;
    sig[3] = r.strict ? 1 : 0;
    sig[4] = r.msg[0];
    r.expect[i] = sig[0] & 1u;
  }
  return r;
}

// 8 threads x `per_thread` requests of 1 to 70 equations (and a few of 0 and of 150); group
// `fail_group` fails on the device
void stress(uint32_t max_requests, uint32_t max_wait_us, int per_thread, long fail_group) {
  constexpr uint32_t CAP = 256, REQ_MAX = 100;
  constexpr int THREADS = 8;
  FakeBackend be(CAP, max_requests ? max_requests : CAP, fail_group, 60);
  nwc::vq::Queue q(be, FakeBackend::NBUF, max_requests, CAP, REQ_MAX, max_wait_us, std::chrono::milliseconds(20));
  std::atomic<uint64_t> answered{0}, errors{0}, grouped{0}, grouped_eq{0}, empty{0}, oversized{0}, expect_redo{0};
  std::vector<std::thread> ts;
  for (int t = 0; t < THREADS; ++t) {
    ts.emplace_back([&, t] {
      std::mt19937 rng(1000 + t);
      for (int k = 0; k < per_thread; ++k) {
        uint32_t n = 1 + rng() % 70;
        if (k % 97 == 5) n = 0;
        if (k % 211 == 7) n = 150;
        Request r = make_request(rng, n, 40, 100000);
        if (t == 0 && k == 0) r.sigs[2] = 1;   // at least one byte the device never writes, in an early group
        std::vector<uint8_t> valid(n + 1, 0xEE);
        const int rc = q.submit(r.msg.data(), r.pks.data(), r.sigs.data(), n, r.strict, valid.data());
        answered.fetch_add(1);
        CHECK(valid[n] == 0xEE);
        if (n == 0) { empty.fetch_add(1); CHECK(rc == 0); continue; }
        if (n > REQ_MAX) oversized.fetch_add(1);
        else { grouped.fetch_add(1); grouped_eq.fetch_add(n); }
        if (rc != 0) {
          // an error code, never "invalid", and no verdict touched
          CHECK(rc == NWC_ERR_DEVICE);
          CHECK(n <= REQ_MAX);
          errors.fetch_add(1);
          continue;
        }
        CHECK(std::equal(r.expect.begin(), r.expect.end(), valid.begin()));   // exactly its own verdicts
        if (n <= REQ_MAX)
          for (uint32_t i = 0; i < n; ++i) expect_redo.fetch_add((r.sigs[64 * i + 1] | r.sigs[64 * i + 2]) & 1u);
      }
    });
  }
  for (std::thread& t : ts) t.join();
  const nwc::vq::Stats st = q.stats();
  CHECK(answered.load() == (uint64_t)THREADS * per_thread);          // every request answered exactly once
  CHECK(st.requests == grouped.load() && st.equations == grouped_eq.load());   // n == 0 and oversized never enter a group
  CHECK(st.bypassed_requests == oversized.load() && be.bypasses.load() == oversized.load());
  CHECK(empty.load() > 0 && oversized.load() > 0);
  CHECK(st.groups == (uint64_t)be.launches.load());
  CHECK(st.max_requests_in_group == be.max_nreq.load());
  CHECK(be.max_nreq.load() <= (max_requests ? max_requests : CAP) && be.max_neq.load() <= CAP);
  if (fail_group >= 0) {
    CHECK(be.launches.load() > fail_group);
    CHECK(errors.load() == be.failed_requests.load() && errors.load() >= 1);   // the failed group's callers, and only they
  } else {
    CHECK(errors.load() == 0);
  }
  // bit-1 and unwritten bytes went through redo, and nothing else did (members of the failed group never poll)
  CHECK(st.redone_equations == be.redo_equations.load());
  CHECK(st.redone_equations >= expect_redo.load() && st.redone_equations > 0);
  CHECK(be.waits.load() > 0);
  CHECK(st.wide_equations <= st.equations && st.cold_equations == 0);
  std::printf("stress max_requests=%u max_wait_us=%u: %llu groups, %llu requests, largest group %llu, %llu redone, %llu waits\n",
              max_requests, max_wait_us, (unsigned long long)st.groups, (unsigned long long)st.requests,
              (unsigned long long)st.max_requests_in_group, (unsigned long long)st.redone_equations,
              (unsigned long long)be.waits.load());
}

// max_requests callers fill one group: a single launch, whatever max_wait_us says
void exact_group() {
  FakeBackend be(256, 8, -1, 0);
  nwc::vq::Queue q(be, FakeBackend::NBUF, 8, 256, 100, 30u * 1000 * 1000);
  std::vector<std::thread> ts;
  for (int t = 0; t < 8; ++t) {
    ts.emplace_back([&, t] {
      std::mt19937 rng(50 + t);
      const Request r = make_request(rng, 1 + t, 0, 0);
      std::vector<uint8_t> valid(1 + t);
      CHECK(q.submit(r.msg.data(), r.pks.data(), r.sigs.data(), 1 + t, r.strict, valid.data()) == 0);
      CHECK(valid == r.expect);
    });
  }
  for (std::thread& t : ts) t.join();
  const nwc::vq::Stats st = q.stats();
  CHECK(st.groups == 1 && st.requests == 8 && st.max_requests_in_group == 8 && st.equations == 36);
  // and a lone caller that never waits is its own group each time
  FakeBackend be1(256, 256, -1, 0);
  nwc::vq::Queue q1(be1, FakeBackend::NBUF, 0, 256, 100, 0);
  std::mt19937 rng(7);
  for (int k = 0; k < 5; ++k) {
    const Request r = make_request(rng, 3, 0, 0);
    std::vector<uint8_t> valid(3);
    CHECK(q1.submit(r.msg.data(), r.pks.data(), r.sigs.data(), 3, r.strict, valid.data()) == 0);
    CHECK(valid == r.expect);
  }
  CHECK(q1.stats().groups == 5 && q1.stats().requests == 5 && q1.stats().max_requests_in_group == 1);
}

// stop() with callers blocked in a group that waits for company: they are launched at once, get
// their answers and have left when stop returns; later calls are refused
void stop_with_blocked_callers() {
  FakeBackend be(256, 64, -1, 0);
  nwc::vq::Queue q(be, FakeBackend::NBUF, 64, 256, 100, 30u * 1000 * 1000);
  std::atomic<int> entered{0}, left{0};
  std::vector<std::thread> ts;
  for (int t = 0; t < 4; ++t) {
    ts.emplace_back([&, t] {
      std::mt19937 rng(90 + t);
      const Request r = make_request(rng, 5, 0, 0);
      std::vector<uint8_t> valid(5);
      entered.fetch_add(1);
      CHECK(q.submit(r.msg.data(), r.pks.data(), r.sigs.data(), 5, r.strict, valid.data()) == 0);
      CHECK(valid == r.expect);
      left.fetch_add(1);
    });
  }
  while (entered.load() < 4) std::this_thread::yield();
  std::this_thread::sleep_for(std::chrono::milliseconds(20));   // let them block inside the group
  const auto t0 = std::chrono::steady_clock::now();
  q.stop();
  CHECK(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(10));   // not the 30 s of max_wait_us
  for (std::thread& t : ts) t.join();
  CHECK(left.load() == 4);
  CHECK(q.stats().requests == 4);
  uint8_t msg[32] = {0}, pk[32] = {0}, sig[64] = {0}, v = 0xEE;
  CHECK(q.submit(msg, pk, sig, 1, true, &v) == NWC_ERR_NOT_INIT && v == 0xEE);
  CHECK(q.submit(msg, pk, sig, 0, true, &v) == 0);
}

}  // namespace

int main(int argc, char** argv) {
  const int per_thread = argc > 1 ? std::atoi(argv[1]) : 2000;
  stress(16, 0, per_thread, 37);         // never wait for company; launch 37 fails
  stress(0, 150, per_thread / 4, -1);    // default cap of requests, wait up to 150 us
  exact_group();
  stop_with_blocked_callers();
  if (g_failures.load()) {
    std::fprintf(stderr, "%llu checks failed\n", (unsigned long long)g_failures.load());
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
