// Drives the vote requests of narwhal_amd/csrc/sanitize_queue.h against a fake backend, on the CPU.
// Built twice by tests/test_sanitize_vote_queue_host.py (thread sanitizer; address + undefined-
// behaviour sanitizers) and run as a child process.  Exit status 0 and a last line "ok" mean every
// check held.
//
// The fake device's code for a message is msg[0] and its kind msg[1] (a message of fewer than two
// bytes: code 8, kind 3).  Further bytes steer the fake and tell it what the caller asked for:
//   msg[2] & 1  the device answers "decide me again" (bit 30)      -> redo, then vote_alone
//   msg[3] & 1  the device never writes the result word            -> wait, redo, then vote_alone
//   msg[4] & 1  the device decides the message but never signs     -> wait, then vote_alone
//   msg[5]      which of the three fake keys the request carries (1..3), 0 = no vote asked: the
//               device checks that the slot's key is exactly that one, so a key left in the buffer
//               by an earlier group would be seen
// The fake "signature" is a function of the message's bytes and the key.
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

constexpr uint64_t KEYS[4] = {0, 0x7f0000001000ull, 0x7f0000002060ull, 0x7f00000030c0ull};

struct Answer {
  int code;
  uint8_t digest[32];
  uint8_t kind;
};
Answer answer_of(const uint8_t* msg, size_t len) {
  Answer a{};
  a.code = len >= 2 ? msg[0] : 8;
  a.kind = len >= 2 ? (uint8_t)(msg[1] & 3) : 3;
  uint32_t sum = 0;
  for (size_t i = 0; i < len; ++i) sum = sum * 31u + msg[i];
  a.digest[0] = (uint8_t)a.code;
  a.digest[1] = a.kind;
  std::memcpy(a.digest + 4, &sum, 4);
  a.digest[31] = 0x5A;
  return a;
}
void sig_of(const uint8_t* msg, size_t len, uint64_t key, uint8_t sig[64]) {
  uint64_t h = key * 0x9E3779B97F4A7C15ull + 1;
  for (size_t i = 0; i < len; ++i) h = (h ^ msg[i]) * 0x100000001B3ull;
  for (int i = 0; i < 64; ++i) {
    h = h * 6364136223846793005ull + 1442695040888963407ull;
    sig[i] = (uint8_t)(h >> 56);
  }
  sig[0] |= 1;   // never all zero
}
bool steer(const uint8_t* msg, size_t len, int at) { return len > (size_t)at && (msg[at] & 1); }
uint64_t key_of(const uint8_t* msg, size_t len) { return len > 5 ? KEYS[msg[5] & 3] : 0; }

struct FakeBackend : nwc::sq::Backend {
  static constexpr int NBUF = 2;
  const uint32_t max_msgs;
  const uint64_t byte_cap;
  const long fail_group;
  const int max_delay_us;
  struct Mem {
    std::vector<uint8_t> data, targets, digests, kinds, vote_sigs, vote_flags;
    std::vector<uint64_t> starts, gc_rounds, vote_keys;
    std::vector<uint32_t> lens, results;
  } mem[NBUF];
  struct Job { int b; uint32_t nmsg; uint64_t nbytes; };
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Job> jobs;
  bool busy[NBUF] = {false, false};
  bool quit = false;
  std::thread device;
  std::atomic<long> launches{0};
  std::atomic<uint64_t> failed_messages{0}, redo_calls{0}, bypasses{0}, alone_calls{0}, signed_in_flight{0}, keyed_slots{0},
      keyless_after_keyed{0};
  bool slot_had_key[NBUF][64] = {};   // device thread only: the slot carried a key in the buffer's previous group

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
      m.vote_keys.resize(max_msgs, 0xDEADull);   // garbage until a member writes its slot
      m.vote_sigs.resize(64 * (size_t)max_msgs);
      m.vote_flags.resize(max_msgs, 0x80);
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
    std::mt19937 rng(4321);
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [&] { return quit || !jobs.empty(); });
      if (jobs.empty()) return;
      const Job j = jobs.front();
      jobs.pop_front();
      lk.unlock();
      if (max_delay_us) std::this_thread::sleep_for(std::chrono::microseconds(rng() % (max_delay_us + 1)));
      Mem& m = mem[j.b];
      for (uint32_t i = 0; i < j.nmsg; ++i) {
        const uint64_t lo = m.starts[i], len = m.lens[i];
        CHECK(lo % 16 == 0 && lo + len <= j.nbytes);
        const uint8_t* msg = &m.data[lo];
        const uint64_t key = m.vote_keys[i];
        // exactly the key its member asked for: a slot that did not ask holds 0, whatever the
        // buffer's previous group left there
        CHECK(key == key_of(msg, len));
        CHECK(__atomic_load_n(&m.results[i], __ATOMIC_RELAXED) == 0);
        CHECK(__atomic_load_n(&m.vote_flags[i], __ATOMIC_RELAXED) == 0);   // the member cleared its flag
        if (i < 64) {
          if (!key && slot_had_key[j.b][i]) keyless_after_keyed.fetch_add(1);
          slot_had_key[j.b][i] = key != 0;
        }
        if (key) keyed_slots.fetch_add(1);
        if (steer(msg, len, 3)) continue;   // left unwritten
        const Answer a = answer_of(msg, len);
        std::memcpy(&m.digests[32 * (size_t)i], a.digest, 32);
        m.kinds[i] = a.kind;
        const bool again = steer(msg, len, 2);
        __atomic_store_n(&m.results[i], nwc::sq::R_WRITTEN | (again ? nwc::sq::R_REDO : 0u) | (3u << 8) | (uint32_t)a.code,
                         __ATOMIC_RELEASE);
        // the vote launch: after the result words, only for Ok headers that carry a key
        if (key && !again && a.code == 0 && a.kind == nwc::sq::KIND_HEADER && !steer(msg, len, 4)) {
          sig_of(msg, len, key, &m.vote_sigs[64 * (size_t)i]);
          signed_in_flight.fetch_add(1);
          __atomic_store_n(&m.vote_flags[i], nwc::sq::VOTE_WRITTEN, __ATOMIC_RELEASE);
        }
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
    g.vote_keys = m.vote_keys.data(); g.vote_sigs = m.vote_sigs.data(); g.vote_flags = m.vote_flags.data();
    return g;
  }
  int launch(int b, uint32_t nmsg, uint64_t nbytes) override {
    CHECK(nmsg >= 1 && nmsg <= max_msgs && nbytes <= byte_cap);
    const long k = launches.fetch_add(1);
    if (k == fail_group) {
      failed_messages.fetch_add(nmsg);
      return NWC_ERR_DEVICE;
    }
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return !busy[b]; });
    busy[b] = true;
    jobs.push_back(Job{b, nmsg, nbytes});
    cv.notify_all();
    return 0;
  }
  int wait(int b) override {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return !busy[b]; });
    return 0;
  }
  static int decide(const uint8_t* msg, size_t len, uint8_t* digest32, uint8_t* kind) {
    const Answer a = answer_of(msg, len);
    if (digest32) std::memcpy(digest32, a.digest, 32);
    if (kind) *kind = a.kind;
    return a.code;
  }
  int redo(const uint8_t* msg, size_t len, uint64_t, const uint8_t*, uint8_t* digest32, uint8_t* kind) override {
    redo_calls.fetch_add(1);
    CHECK(steer(msg, len, 2) || steer(msg, len, 3));
    return decide(msg, len, digest32, kind);
  }
  int bypass(const uint8_t* msg, size_t len, uint64_t, const uint8_t*, uint8_t* digest32, uint8_t* kind) override {
    bypasses.fetch_add(1);
    return decide(msg, len, digest32, kind);
  }
  int vote_alone(const uint8_t* msg, size_t len, const uint8_t* id32, uint64_t vote_key, uint8_t* sig64) override {
    alone_calls.fetch_add(1);
    const Answer a = answer_of(msg, len);
    // never speculatively: only for a message already decided Ok + header, with the key it asked for
    CHECK(a.code == 0 && a.kind == nwc::sq::KIND_HEADER);
    CHECK(vote_key != 0 && vote_key == key_of(msg, len));
    CHECK(std::memcmp(id32, a.digest, 32) == 0);
    CHECK(len > byte_cap || steer(msg, len, 2) || steer(msg, len, 3) || steer(msg, len, 4) || (len > 6 && msg[6] == 0xD1));
    sig_of(msg, len, vote_key, sig64);
    return 0;
  }
};

struct Request {
  std::vector<uint8_t> msg;
  uint64_t key;
};
Request make_request(std::mt19937& rng, size_t len, bool ask, int steer_one_in) {
  Request r;
  r.msg.resize(len);
  for (uint8_t& x : r.msg) x = (uint8_t)rng();
  if (len > 0) r.msg[0] = rng() % 3 ? 0 : (uint8_t)(rng() % 12);   // mostly Ok
  if (len > 1) r.msg[1] = rng() % 3 ? 0 : (uint8_t)(rng() % 4);    // mostly headers
  for (size_t k = 2; k <= 4 && k < len; ++k) r.msg[k] = steer_one_in && rng() % steer_one_in == 0;
  if (len > 5) r.msg[5] = ask ? (uint8_t)(1 + rng() % 3) : 0;
  if (len > 6) r.msg[6] = 0;
  r.key = key_of(r.msg.data(), len);
  return r;
}
// What the caller must see; returns rc.  *voted_out: the caller got a vote.
int submit_checked(nwc::sq::Queue& q, const Request& r, bool* voted_out, bool direct = false) {
  uint8_t digest[32], kind = 0xEE, sig[65];
  int voted = 77;
  std::memset(digest, 0xEE, sizeof digest);
  std::memset(sig, 0xEE, sizeof sig);
  const uint8_t* p = r.msg.data();
  const size_t len = r.msg.size();
  const int rc = r.key ? q.submit(p, len, 5, nullptr, digest, &kind, direct, r.key, sig, &voted)
                       : q.submit(p, len, 5, nullptr, digest, &kind, direct);
  const Answer a = answer_of(p, len);
  static const uint8_t zero[64] = {0};
  *voted_out = false;
  if (!r.key) {
    CHECK(voted == 77 && sig[0] == 0xEE);   // outputs it did not pass are not touched
  } else {
    CHECK(sig[64] == 0xEE);
    const bool expect = rc >= 0 && a.code == 0 && a.kind == nwc::sq::KIND_HEADER;   // asked and Ok and a header
    CHECK(voted == (expect ? 1 : 0));
    if (expect) {
      uint8_t want[64];
      sig_of(p, len, r.key, want);   // its own: this message under this key
      CHECK(std::memcmp(sig, want, 64) == 0);
    } else {
      CHECK(std::memcmp(sig, zero, 64) == 0);
    }
    *voted_out = voted == 1;
  }
  if (rc < 0) {
    CHECK(digest[0] == 0xEE && kind == 0xEE);
    return rc;
  }
  CHECK(rc == a.code && std::memcmp(digest, a.digest, 32) == 0 && kind == a.kind);
  return rc;
}

// 8 threads x per_thread requests, half of them asking for a vote with one of three keys
void stress(uint32_t max_messages, uint32_t max_wait_us, int per_thread, long fail_group) {
  constexpr uint32_t MSG_CAP = 64;
  constexpr uint64_t BYTE_CAP = 16 << 10;
  constexpr int THREADS = 8;
  FakeBackend be(max_messages ? max_messages : MSG_CAP, BYTE_CAP, fail_group, 60);
  nwc::sq::Queue q(be, FakeBackend::NBUF, max_messages, MSG_CAP, BYTE_CAP, max_wait_us, std::chrono::milliseconds(20));
  std::atomic<uint64_t> answered{0}, errors{0}, votes{0}, expect_alone{0}, asked_in_groups{0}, oversized_voted{0};
  std::vector<std::thread> ts;
  for (int t = 0; t < THREADS; ++t) {
    ts.emplace_back([&, t] {
      std::mt19937 rng(3000 + t);
      for (int k = 0; k < per_thread; ++k) {
        size_t len = 7 + rng() % 3000;
        if (k % 97 == 5) len = rng() % 6;          // too short to ask, the empty message among them
        if (k % 211 == 7) len = BYTE_CAP + 1 + rng() % 100;
        Request r = make_request(rng, len, (k & 1) != 0, 60);
        if (t == 0 && k == 1) { r.msg[0] = 0; r.msg[1] = 0; r.msg[2] = 0; r.msg[3] = 0; r.msg[4] = 1; }   // one unsigned Ok header early
        if (t == 1 && k == 1) { r.msg[0] = 0; r.msg[1] = 0; r.msg[2] = 0; r.msg[3] = 1; }                 // one unwritten word
        if (t == 2 && k == 1) { r.msg[0] = 0; r.msg[1] = 0; r.msg[2] = 1; r.msg[3] = 0; }                 // one redo word
        bool voted = false;
        const int rc = submit_checked(q, r, &voted);
        answered.fetch_add(1);
        if (rc < 0) {
          CHECK(rc == NWC_ERR_DEVICE && !voted && len <= BYTE_CAP);   // a failed launch: the error and no vote
          errors.fetch_add(1);
          continue;
        }
        if (len <= BYTE_CAP && r.key) asked_in_groups.fetch_add(1);
        if (!voted) continue;
        votes.fetch_add(1);
        const uint8_t* p = r.msg.data();
        if (len > BYTE_CAP) { oversized_voted.fetch_add(1); expect_alone.fetch_add(1); }
        else if (steer(p, len, 2) || steer(p, len, 3) || steer(p, len, 4)) expect_alone.fetch_add(1);
      }
    });
  }
  for (std::thread& t : ts) t.join();
  const nwc::sq::Stats st = q.stats();
  CHECK(answered.load() == (uint64_t)THREADS * per_thread);
  CHECK(votes.load() > 0 && expect_alone.load() > 0 && oversized_voted.load() > 0);
  // unwritten flags, redo words and oversized messages reached vote_alone exactly once each
  CHECK(be.alone_calls.load() == expect_alone.load() && st.votes_alone == expect_alone.load());
  CHECK(st.votes_in_flight == votes.load() - expect_alone.load());
  CHECK(be.signed_in_flight.load() == st.votes_in_flight);   // what the device signed, its callers took
  CHECK(be.keyless_after_keyed.load() > 0);   // buffer reuse after a voting group was exercised
  if (fail_group >= 0) CHECK(errors.load() == be.failed_messages.load() && errors.load() >= 1);
  else CHECK(errors.load() == 0);
  CHECK(st.redone_messages == be.redo_calls.load());
  std::printf("stress max_messages=%u max_wait_us=%u: %llu groups, %llu messages, %llu votes in flight, %llu alone, %llu errors\n",
              max_messages, max_wait_us, (unsigned long long)st.groups, (unsigned long long)st.messages,
              (unsigned long long)st.votes_in_flight, (unsigned long long)st.votes_alone, (unsigned long long)errors.load());
}

// a voting group of 8 fills a buffer; the groups after it on the same buffers ask for nothing and
// must present key 0 in every slot (the device checks each slot against what its message asked)
void stale_keys() {
  FakeBackend be(8, 64 << 10, -1, 0);
  nwc::sq::Queue q(be, FakeBackend::NBUF, 8, 8, 64 << 10, 30u * 1000 * 1000);
  for (int round = 0; round < 6; ++round) {
    const bool ask = round % 3 == 0;
    std::vector<std::thread> ts;
    for (int t = 0; t < 8; ++t) {
      ts.emplace_back([&, t] {
        std::mt19937 rng(50 + 8 * round + t);
        Request r = make_request(rng, 40 + 13 * t, ask, 0);
        r.msg[0] = 0;
        r.msg[1] = 0;
        bool voted = false;
        CHECK(submit_checked(q, r, &voted) == 0 && voted == ask);
      });
    }
    for (std::thread& t : ts) t.join();
  }
  const nwc::sq::Stats st = q.stats();
  CHECK(st.groups == 6 && st.votes_in_flight == 16 && st.votes_alone == 0);
  CHECK(be.keyed_slots.load() == 16 && be.keyless_after_keyed.load() >= 8);
  // `direct` goes round the groups: the vote comes from vote_alone, and only for an Ok header
  std::mt19937 rng(9);
  Request d = make_request(rng, 100, true, 0);
  d.msg[0] = 0; d.msg[1] = 0; d.msg[6] = 0xD1;
  bool voted = false;
  CHECK(submit_checked(q, d, &voted, true) == 0 && voted);
  d.msg[0] = 1;   // an invalid signature: no vote, vote_alone not asked
  CHECK(submit_checked(q, d, &voted, true) == 1 && !voted);
  d.msg[0] = 0; d.msg[1] = 2;   // a certificate
  CHECK(submit_checked(q, d, &voted, true) == 0 && !voted);
  CHECK(q.stats().votes_alone == 1 && be.alone_calls.load() == 1);
  // a key without outputs is refused before anything is queued
  CHECK(q.submit(d.msg.data(), d.msg.size(), 0, nullptr, nullptr, nullptr, false, KEYS[1], nullptr, nullptr) == NWC_ERR_ARG);
}

// a backend without votes (the default vote_alone): an Ok header that needs the fallback gets the error
void backend_without_votes() {
  struct NoVotes : FakeBackend {
    using FakeBackend::FakeBackend;
    int vote_alone(const uint8_t* a, size_t b, const uint8_t* c, uint64_t d, uint8_t* e) override {
      return nwc::sq::Backend::vote_alone(a, b, c, d, e);
    }
  } be(8, 4096, -1, 0);
  nwc::sq::Queue q(be, FakeBackend::NBUF, 0, 8, 4096, 0, std::chrono::milliseconds(5));
  std::mt19937 rng(3);
  Request r = make_request(rng, 64, true, 0);
  r.msg[0] = 0; r.msg[1] = 0; r.msg[4] = 1;   // decided, never signed
  uint8_t dig[32], kind = 0xEE, sig[64];
  std::memset(dig, 0xEE, 32);
  int voted = 5;
  CHECK(q.submit(r.msg.data(), r.msg.size(), 0, nullptr, dig, &kind, false, r.key, sig, &voted) == NWC_ERR_ARG);
  static const uint8_t zero[64] = {0};
  CHECK(voted == 0 && std::memcmp(sig, zero, 64) == 0 && kind == 0xEE && dig[0] == 0xEE);
}

// stop() with voters blocked in a group that waits for company: launched at once, every voter gets
// its vote and has left when stop returns
void stop_with_blocked_voters() {
  FakeBackend be(64, 64 << 10, -1, 0);
  nwc::sq::Queue q(be, FakeBackend::NBUF, 64, 64, 64 << 10, 30u * 1000 * 1000);
  std::atomic<int> left{0};
  std::vector<std::thread> ts;
  for (int t = 0; t < 4; ++t) {
    ts.emplace_back([&, t] {
      std::mt19937 rng(90 + t);
      Request r = make_request(rng, 500, true, 0);
      r.msg[0] = 0;
      r.msg[1] = 0;
      bool voted = false;
      CHECK(submit_checked(q, r, &voted) == 0 && voted);
      left.fetch_add(1);
    });
  }
  while (q.stats().messages < 4) std::this_thread::yield();
  const auto t0 = std::chrono::steady_clock::now();
  q.stop();
  CHECK(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(10));
  for (std::thread& t : ts) t.join();
  CHECK(left.load() == 4 && q.stats().groups == 1 && q.stats().votes_in_flight == 4);
  uint8_t msg[8] = {0}, sig[64];
  int voted = 9;
  std::memset(sig, 0xEE, 64);
  CHECK(q.submit(msg, 8, 0, nullptr, nullptr, nullptr, false, KEYS[1], sig, &voted) == NWC_ERR_NOT_INIT && voted == 0 && sig[0] == 0);
}

}  // namespace

int main(int argc, char** argv) {
  const int per_thread = argc > 1 ? std::atoi(argv[1]) : 2000;
  stress(16, 0, per_thread, 37);
  stress(0, 150, per_thread / 4, -1);
  stale_keys();
  backend_without_votes();
  stop_with_blocked_voters();
  if (g_failures.load()) {
    std::fprintf(stderr, "%llu checks failed\n", (unsigned long long)g_failures.load());
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
