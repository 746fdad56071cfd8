// Drives narwhal_amd/csrc/sanitize_queue.h against a fake backend, on the CPU.  Built twice by
// tests/test_sanitize_queue_host.py (thread sanitizer; address + undefined-behaviour sanitizers) and
// run as a child process.  Exit status 0 and a last line "ok" mean every check held.
//
// The fake device's code for a message is its first byte (a message of no bytes: 8, the
// serialization error).  Further bytes steer the fake:
//   msg[1] & 1  the device answers "decide me again" (bit 30) -> the queue must call redo
//   msg[2] & 1  the device never writes the word -> poll time-out, wait, then redo
// The digest the fake returns carries what the caller can check: the code, the low byte of the
// request's gc_round, the first byte of its vote target (0xAA without one), the length and a sum
// over every byte of the message as it lay in the group buffer; the kind is msg[0] % 4.
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

#include "sanitize_queue.h"

namespace {

using nwc::sq::GroupBuf;

std::atomic<uint64_t> g_failures{0};
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      g_failures.fetch_add(1);                                           \
    }                                                                    \
  } while (0)

struct Answer {
  int code;
  uint8_t digest[32];
  uint8_t kind;
};
// what every route (group, redo, bypass) answers for a message
Answer answer_of(const uint8_t* msg, size_t len, uint64_t gc_round, const uint8_t* target) {
  Answer a{};
  a.code = len ? msg[0] : 8;
  uint32_t sum = 0;
  for (size_t i = 0; i < len; ++i) sum = sum * 31u + msg[i];
  a.digest[0] = (uint8_t)a.code;
  a.digest[1] = (uint8_t)gc_round;
  a.digest[2] = target ? target[0] : 0xAA;
  a.digest[3] = (uint8_t)len;
  a.digest[4] = (uint8_t)(len >> 8);
  a.digest[5] = (uint8_t)(len >> 16);
  std::memcpy(a.digest + 8, &sum, 4);
  a.digest[31] = 0x5A;
  a.kind = (uint8_t)(a.code % 4);
  return a;
}

struct FakeBackend : nwc::sq::Backend {
  static constexpr int NBUF = 2;
  const uint32_t max_msgs;
  const uint64_t byte_cap;
  const long fail_group;   // index of the launch that fails (-1 = none)
  const int max_delay_us;
  struct Mem {
    std::vector<uint8_t> data, targets, digests, kinds;
    std::vector<uint64_t> starts, gc_rounds;
    std::vector<uint32_t> lens, results;
  } mem[NBUF];
  // the fake device: one thread, launches complete in order after a random delay
  struct Job { int b; uint32_t nmsg; uint64_t nbytes; };
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Job> jobs;
  bool busy[NBUF] = {false, false};
  bool quit = false;
  std::thread device;
  std::atomic<long> launches{0};
  std::atomic<uint64_t> failed_messages{0}, redo_calls{0}, waits{0}, bypasses{0}, max_nmsg{0}, max_nbytes{0};

  FakeBackend(uint32_t max_msgs_, uint64_t byte_cap_, long fail_group_, int max_delay_us_)
      : max_msgs(max_msgs_), byte_cap(byte_cap_), fail_group(fail_group_), max_delay_us(max_delay_us_) {
    for (Mem& m : mem) {
      m.data.resize(byte_cap + 16);
      m.starts.resize(max_msgs);
      m.lens.resize(max_msgs);
      m.gc_rounds.resize(max_msgs);
      m.targets.resize(nwc::sq::TARGET_STRIDE * (size_t)max_msgs);
      m.results.resize(max_msgs);
      m.digests.resize(32 * (size_t)max_msgs);
      m.kinds.resize(max_msgs);
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
      uint64_t prev_end = 0;
      for (uint32_t i = 0; i < j.nmsg; ++i) {
        const uint64_t lo = m.starts[i], len = m.lens[i];
        CHECK(lo % 16 == 0);                       // every range starts 16-byte aligned
        CHECK(lo >= prev_end);                     // in slot order, so no two overlap
        CHECK(lo + len <= j.nbytes && j.nbytes <= byte_cap);
        prev_end = lo + len;
        CHECK(__atomic_load_n(&m.results[i], __ATOMIC_RELAXED) == 0);   // the member cleared its word
        const uint8_t* msg = &m.data[lo];
        const uint8_t* t = &m.targets[nwc::sq::TARGET_STRIDE * (size_t)i];
        CHECK(t[nwc::sq::TARGET_FLAG_AT] <= 1);
        const Answer a = answer_of(msg, len, m.gc_rounds[i], t[nwc::sq::TARGET_FLAG_AT] ? t : nullptr);
        if (len > 2 && (msg[2] & 1)) continue;     // left unwritten
        std::memcpy(&m.digests[32 * (size_t)i], a.digest, 32);
        m.kinds[i] = a.kind;
        const bool again = len > 1 && (msg[1] & 1);
        const uint32_t w = nwc::sq::R_WRITTEN | (again ? nwc::sq::R_REDO : 0u) | (3u << 8) | (uint32_t)a.code;
        __atomic_store_n(&m.results[i], w, __ATOMIC_RELEASE);
      }
      lk.lock();
      busy[j.b] = false;
      cv.notify_all();
    }
  }

  GroupBuf buffer(int b) override {
    Mem& m = mem[b];
    GroupBuf g;
    g.data = m.data.data(); g.starts = m.starts.data(); g.lens = m.lens.data(); g.gc_rounds = m.gc_rounds.data();
    g.targets = m.targets.data(); g.results = m.results.data(); g.digests = m.digests.data(); g.kinds = m.kinds.data();
    return g;
  }
  int launch(int b, uint32_t nmsg, uint64_t nbytes) override {
    CHECK(nmsg >= 1 && nmsg <= max_msgs);
    CHECK(nbytes <= byte_cap);
    uint64_t prev = max_nmsg.load();
    while (nmsg > prev && !max_nmsg.compare_exchange_weak(prev, nmsg)) {}
    prev = max_nbytes.load();
    while (nbytes > prev && !max_nbytes.compare_exchange_weak(prev, nbytes)) {}
    const long k = launches.fetch_add(1);
    if (k == fail_group) {
      failed_messages.fetch_add(nmsg);
      return NWC_ERR_DEVICE;
    }
    // a buffer is launched again only after its members have all left, that is after the device
    // has stored its last word; the device thread may still be on its way out of that job (a
    // stream orders the next launch behind it)
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return !busy[b]; });
    busy[b] = true;
    jobs.push_back(Job{b, nmsg, nbytes});
    cv.notify_all();
    return 0;
  }
  int wait(int b) override {
    waits.fetch_add(1);
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return !busy[b]; });
    return 0;
  }
  static int decide(const uint8_t* msg, size_t len, uint64_t gc_round, const uint8_t* target, uint8_t* digest32, uint8_t* kind) {
    const Answer a = answer_of(msg, len, gc_round, target);
    if (digest32) std::memcpy(digest32, a.digest, 32);
    if (kind) *kind = a.kind;
    return a.code;
  }
  int redo(const uint8_t* msg, size_t len, uint64_t gc_round, const uint8_t* target, uint8_t* digest32, uint8_t* kind) override {
    redo_calls.fetch_add(1);
    CHECK(len > 1 && ((msg[1] & 1) || (len > 2 && (msg[2] & 1))));   // only messages that asked for it, or were left unwritten
    return decide(msg, len, gc_round, target, digest32, kind);
  }
  int bypass(const uint8_t* msg, size_t len, uint64_t gc_round, const uint8_t* target, uint8_t* digest32, uint8_t* kind) override {
    bypasses.fetch_add(1);
    return decide(msg, len, gc_round, target, digest32, kind);
  }
};

struct Request {
  std::vector<uint8_t> msg, target;
  uint64_t gc_round;
  bool has_target;
};
Request make_request(std::mt19937& rng, size_t len, int redo_one_in, int lost_one_in) {
  Request r;
  r.msg.resize(len);
  for (uint8_t& x : r.msg) x = (uint8_t)rng();
  if (len > 0) r.msg[0] = (uint8_t)(rng() % 12);   // a NWC_DAG_* code
  if (len > 1) r.msg[1] = redo_one_in && rng() % redo_one_in == 0;
  if (len > 2) r.msg[2] = lost_one_in && rng() % lost_one_in == 0;
  r.gc_round = rng();
  r.has_target = rng() & 1;
  r.target.resize(72);
  for (uint8_t& x : r.target) x = (uint8_t)rng();
  return r;
}
// submits r and checks that the caller got exactly its own code, digest and kind; returns the code or error
int submit_checked(nwc::sq::Queue& q, const Request& r, bool direct = false) {
  uint8_t digest[33], kind[2] = {0xEE, 0xEE};
  std::memset(digest, 0xEE, sizeof digest);
  const uint8_t* t = r.has_target ? r.target.data() : nullptr;
  const int rc = q.submit(r.msg.data(), r.msg.size(), r.gc_round, t, digest, kind, direct);
  CHECK(digest[32] == 0xEE && kind[1] == 0xEE);
  if (rc < 0) {
    CHECK(digest[0] == 0xEE && kind[0] == 0xEE);   // an error touches no output
    return rc;
  }
  const Answer a = answer_of(r.msg.data(), r.msg.size(), r.gc_round, t);
  CHECK(rc == a.code);
  CHECK(std::memcmp(digest, a.digest, 32) == 0);
  CHECK(kind[0] == a.kind);
  return rc;
}

// 8 threads x `per_thread` messages of 1 to 20,000 bytes (and a few of 0 and of 70,000); group
// `fail_group` fails on the device
void stress(uint32_t max_messages, uint32_t max_wait_us, int per_thread, long fail_group) {
  constexpr uint32_t MSG_CAP = 64;
  constexpr uint64_t BYTE_CAP = 64 << 10;
  constexpr int THREADS = 8;
  FakeBackend be(max_messages ? max_messages : MSG_CAP, BYTE_CAP, fail_group, 60);
  nwc::sq::Queue q(be, FakeBackend::NBUF, max_messages, MSG_CAP, BYTE_CAP, max_wait_us, std::chrono::milliseconds(20));
  std::atomic<uint64_t> answered{0}, errors{0}, grouped{0}, grouped_bytes{0}, empty{0}, oversized{0}, expect_redo{0};
  std::vector<std::thread> ts;
  for (int t = 0; t < THREADS; ++t) {
    ts.emplace_back([&, t] {
      std::mt19937 rng(1000 + t);
      for (int k = 0; k < per_thread; ++k) {
        size_t len = 1 + rng() % 20000;
        if (rng() % 3 == 0) len = 1 + rng() % 300;   // vote-sized ones, so that groups fill with many messages
        if (k % 97 == 5) len = 0;
        if (k % 211 == 7) len = 70000;
        Request r = make_request(rng, len, 40, 100000);
        if (t == 0 && k == 0) r.msg[2] = 1;   // at least one word the device never writes, in an early group
        const int rc = submit_checked(q, r);
        answered.fetch_add(1);
        if (len == 0) empty.fetch_add(1);
        if (len > BYTE_CAP) { oversized.fetch_add(1); CHECK(rc >= 0); continue; }
        grouped.fetch_add(1);
        grouped_bytes.fetch_add(len);
        if (rc < 0) {
          CHECK(rc == NWC_ERR_DEVICE);   // an error code, never a NWC_DAG_* code
          errors.fetch_add(1);
          continue;
        }
        if (len > 1) expect_redo.fetch_add((r.msg[1] | (len > 2 ? r.msg[2] : 0)) & 1u);
      }
    });
  }
  for (std::thread& t : ts) t.join();
  const nwc::sq::Stats st = q.stats();
  CHECK(answered.load() == (uint64_t)THREADS * per_thread);          // every request answered exactly once
  CHECK(st.messages == grouped.load() && st.bytes == grouped_bytes.load());   // oversized messages never enter a group
  CHECK(st.bypassed_messages == oversized.load() && be.bypasses.load() == oversized.load());
  CHECK(empty.load() > 0 && oversized.load() > 0);
  CHECK(st.groups == (uint64_t)be.launches.load());
  CHECK(st.max_messages_in_group == be.max_nmsg.load() && st.max_messages_in_group > 1);
  CHECK(be.max_nmsg.load() <= (max_messages ? max_messages : MSG_CAP) && be.max_nbytes.load() <= BYTE_CAP);
  if (fail_group >= 0) {
    CHECK(be.launches.load() > fail_group);
    CHECK(errors.load() == be.failed_messages.load() && errors.load() >= 1);   // the failed group's callers, and only they
  } else {
    CHECK(errors.load() == 0);
  }
  // redo-bit and unwritten words went through redo, and nothing else did (members of the failed group never poll)
  CHECK(st.redone_messages == be.redo_calls.load());
  CHECK(st.redone_messages == expect_redo.load() && st.redone_messages > 0);
  CHECK(be.waits.load() > 0);
  CHECK(st.equations == 3 * (st.messages - errors.load() - st.redone_messages));   // the words' equation counts
  std::printf("stress max_messages=%u max_wait_us=%u: %llu groups, %llu messages, largest group %llu, %llu redone, %llu waits\n",
              max_messages, max_wait_us, (unsigned long long)st.groups, (unsigned long long)st.messages,
              (unsigned long long)st.max_messages_in_group, (unsigned long long)st.redone_messages,
              (unsigned long long)be.waits.load());
}

// max_messages callers fill one group: a single launch, whatever max_wait_us says
void exact_group() {
  FakeBackend be(8, 64 << 10, -1, 0);
  nwc::sq::Queue q(be, FakeBackend::NBUF, 8, 8, 64 << 10, 30u * 1000 * 1000);
  std::vector<std::thread> ts;
  for (int t = 0; t < 8; ++t) {
    ts.emplace_back([&, t] {
      std::mt19937 rng(50 + t);
      const Request r = make_request(rng, 5 + 37 * t, 0, 0);   // lengths that are no multiple of 4 or 16
      CHECK(submit_checked(q, r) >= 0);
    });
  }
  for (std::thread& t : ts) t.join();
  const nwc::sq::Stats st = q.stats();
  CHECK(st.groups == 1 && st.messages == 8 && st.max_messages_in_group == 8 && st.redone_messages == 0);
  // a lone caller that never waits is its own group each time; `direct` goes round the groups
  FakeBackend be1(64, 4096, -1, 0);
  nwc::sq::Queue q1(be1, FakeBackend::NBUF, 0, 64, 4096, 0);
  std::mt19937 rng(7);
  for (int k = 0; k < 5; ++k) CHECK(submit_checked(q1, make_request(rng, 100 + k, 0, 0)) >= 0);
  CHECK(q1.stats().groups == 5 && q1.stats().messages == 5 && q1.stats().max_messages_in_group == 1);
  CHECK(submit_checked(q1, make_request(rng, 100, 0, 0), true) >= 0);
  CHECK(submit_checked(q1, make_request(rng, 4096, 0, 0)) >= 0);   // exactly a group's bytes: grouped
  CHECK(submit_checked(q1, make_request(rng, 4097, 0, 0)) >= 0);   // one more: bypassed
  CHECK(q1.stats().groups == 6 && q1.stats().bypassed_messages == 2 && be1.bypasses.load() == 2);
}

// the second message does not fit behind the first: two groups, the first closed by the second's arrival
void byte_capacity_closes_a_group() {
  FakeBackend be(8, 4096, -1, 0);
  nwc::sq::Queue q(be, FakeBackend::NBUF, 8, 8, 4096, 300 * 1000);
  std::mt19937 rng(11);
  const Request a = make_request(rng, 3000, 0, 0), b = make_request(rng, 2000, 0, 0);
  std::thread ta([&] { CHECK(submit_checked(q, a) >= 0); });
  while (q.stats().messages < 1) std::this_thread::yield();
  const auto t0 = std::chrono::steady_clock::now();
  CHECK(submit_checked(q, b) >= 0);
  ta.join();
  (void)t0;
  CHECK(q.stats().groups == 2 && q.stats().max_messages_in_group == 1 && be.max_nbytes.load() <= 4096);
}

// stop() with callers blocked in a group that waits for company: they are launched at once, get
// their answers and have left when stop returns; later calls are refused
void stop_with_blocked_callers() {
  FakeBackend be(64, 64 << 10, -1, 0);
  nwc::sq::Queue q(be, FakeBackend::NBUF, 64, 64, 64 << 10, 30u * 1000 * 1000);
  std::atomic<int> left{0};
  std::vector<std::thread> ts;
  for (int t = 0; t < 4; ++t) {
    ts.emplace_back([&, t] {
      std::mt19937 rng(90 + t);
      CHECK(submit_checked(q, make_request(rng, 500, 0, 0)) >= 0);
      left.fetch_add(1);
    });
  }
  while (q.stats().messages < 4) std::this_thread::yield();   // all four have joined the group
  const auto t0 = std::chrono::steady_clock::now();
  q.stop();
  CHECK(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(10));   // not the 30 s of max_wait_us
  CHECK(q.stats().groups == 1);   // stop returned after they had been launched and had left the queue
  for (std::thread& t : ts) t.join();
  CHECK(left.load() == 4);
  CHECK(q.stats().messages == 4 && q.stats().groups == 1);
  uint8_t msg[4] = {0}, dig[32], kind = 0xEE;
  std::memset(dig, 0xEE, 32);
  CHECK(q.submit(msg, 4, 0, nullptr, dig, &kind) == NWC_ERR_NOT_INIT && kind == 0xEE && dig[0] == 0xEE);
}

}  // namespace

int main(int argc, char** argv) {
  const int per_thread = argc > 1 ? std::atoi(argv[1]) : 2000;
  stress(16, 0, per_thread, 37);         // never wait for company; launch 37 fails
  stress(0, 150, per_thread / 4, -1);    // default cap of messages, wait up to 150 us
  exact_group();
  byte_capacity_closes_a_group();
  stop_with_blocked_callers();
  if (g_failures.load()) {
    std::fprintf(stderr, "%llu checks failed\n", (unsigned long long)g_failures.load());
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
