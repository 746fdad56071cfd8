// Drives the view requests of narwhal_amd/csrc/sanitize_queue.h against a fake backend, on the CPU.
// Built twice by tests/test_sanitize_view_queue_host.py (thread sanitizer; address + undefined-
// behaviour sanitizers) and run as a child process.  Exit status 0 and a last line "ok" mean every
// check held.
//
// The fake device's code for a message is msg[0] and its kind msg[1] (a message of fewer than two
// bytes: code 8, kind 3).  Further bytes steer the fake and tell it what the caller asked for:
//   msg[2] & 1  the device answers "decide me again" (bit 30)      -> view_alone (not redo)
//   msg[3] & 1  the device never writes the result word            -> wait, view_alone (not redo)
//   msg[4] & 1  the device decides the message but never signs     -> wait, then vote_alone
//   msg[5]      which of the three fake keys the request carries (1..3), 0 = no vote asked
//   msg[6]      0xD1 marks a request submitted with `direct`
//   msg[7] & 1  the request asks for a view: the device checks that the slot's wanted byte says
//               exactly that, so a byte left in the buffer by an earlier group would be seen
//   msg[8] & 1  the device decides the message but never writes the view flag -> wait, view_alone
// The fake record, body length and body are functions of the message's bytes.
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
using nwc::sq::VIEW_BYTES;
using nwc::sq::ViewReq;

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
uint64_t hash_of(const uint8_t* msg, size_t len, uint64_t salt) {
  uint64_t h = salt * 0x9E3779B97F4A7C15ull + 1;
  for (size_t i = 0; i < len; ++i) h = (h ^ msg[i]) * 0x100000001B3ull;
  return h;
}
void fill(uint8_t* out, size_t n, uint64_t h) {
  for (size_t i = 0; i < n; ++i) {
    h = h * 6364136223846793005ull + 1442695040888963407ull;
    out[i] = (uint8_t)(h >> 56);
  }
}
void sig_of(const uint8_t* msg, size_t len, uint64_t key, uint8_t sig[64]) {
  fill(sig, 64, hash_of(msg, len, key));
  sig[0] |= 1;   // never all zero
}
// the fake view: decoded = 1, the kind, the code, then bytes that depend on the whole message; a
// body of up to the bound (len + 64) bytes, the bound itself among the lengths
void record_of(const uint8_t* msg, size_t len, uint8_t rec[VIEW_BYTES]) {
  const Answer a = answer_of(msg, len);
  fill(rec, VIEW_BYTES, hash_of(msg, len, 0xABCD));
  rec[0] = 1;
  rec[1] = a.kind;
  const int32_t code = a.code;
  std::memcpy(rec + 4, &code, 4);
}
uint32_t body_len_of(const uint8_t* msg, size_t len) {
  const uint64_t h = hash_of(msg, len, 0xB0D7);
  if (h % 7 == 0) return 0;
  if (h % 7 == 1) return (uint32_t)nwc::sq::view_body_bound(len);
  return (uint32_t)((h >> 8) % (nwc::sq::view_body_bound(len) + 1));
}
void body_of(const uint8_t* msg, size_t len, uint8_t* body) { fill(body, body_len_of(msg, len), hash_of(msg, len, 0xB0D8)); }

bool steer(const uint8_t* msg, size_t len, int at) { return len > (size_t)at && (msg[at] & 1); }
uint64_t key_of(const uint8_t* msg, size_t len) { return len > 5 ? KEYS[msg[5] & 3] : 0; }
bool asks_view(const uint8_t* msg, size_t len) { return steer(msg, len, 7); }

struct FakeBackend : nwc::sq::Backend {
  static constexpr int NBUF = 2;
  const uint32_t max_msgs;
  const uint64_t byte_cap;
  const long fail_group;
  const int max_delay_us;
  struct Mem {
    std::vector<uint8_t> data, targets, digests, kinds, vote_sigs, vote_flags, view_wanted, views, view_flags, view_body;
    std::vector<uint64_t> starts, gc_rounds, vote_keys;
    std::vector<uint32_t> lens, results, view_used;
  } mem[NBUF];
  struct Job { int b; uint32_t nmsg; uint64_t nbytes; };
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Job> jobs;
  bool busy[NBUF] = {false, false};
  bool quit = false;
  std::thread device;
  std::atomic<long> launches{0};
  std::atomic<uint64_t> failed_messages{0}, redo_calls{0}, bypasses{0}, vote_alone_calls{0}, view_alone_calls{0},
      built_in_flight{0}, wanted_slots{0}, unwanted_after_wanted{0};
  bool slot_wanted[NBUF][64] = {};   // device thread only: the slot asked in the buffer's previous group

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
      m.view_wanted.resize(max_msgs, 0xDE);
      m.views.resize(VIEW_BYTES * (size_t)max_msgs, 0xDE);
      m.view_used.resize(max_msgs, 0xDEDEDEDEu);
      m.view_flags.resize(max_msgs, 0x80);
      m.view_body.resize(byte_cap + nwc::sq::VIEW_SLACK * max_msgs);   // exactly the documented size
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
        const uint8_t wanted = m.view_wanted[i];
        // exactly what its member asked for: a slot that did not ask holds 0, whatever the
        // buffer's previous group left there
        CHECK(key == key_of(msg, len));
        CHECK((wanted != 0) == asks_view(msg, len));
        CHECK(__atomic_load_n(&m.results[i], __ATOMIC_RELAXED) == 0);
        CHECK(__atomic_load_n(&m.vote_flags[i], __ATOMIC_RELAXED) == 0);
        CHECK(__atomic_load_n(&m.view_flags[i], __ATOMIC_RELAXED) == 0);   // the member cleared its flag
        if (i < 64) {
          if (!wanted && slot_wanted[j.b][i]) unwanted_after_wanted.fetch_add(1);
          slot_wanted[j.b][i] = wanted != 0;
        }
        if (wanted) wanted_slots.fetch_add(1);
        if (steer(msg, len, 3)) continue;   // left unwritten
        const Answer a = answer_of(msg, len);
        std::memcpy(&m.digests[32 * (size_t)i], a.digest, 32);
        m.kinds[i] = a.kind;
        const bool again = steer(msg, len, 2);
        __atomic_store_n(&m.results[i], nwc::sq::R_WRITTEN | (again ? nwc::sq::R_REDO : 0u) | (3u << 8) | (uint32_t)a.code,
                         __ATOMIC_RELEASE);
        // the view launch: after the result words, for every decided slot that asks, whatever its code
        if (wanted && !again && !steer(msg, len, 8)) {
          const uint64_t at = nwc::sq::view_region(lo, i);
          const uint32_t used = body_len_of(msg, len);
          CHECK(at + nwc::sq::view_body_bound(len) <= m.view_body.size());
          record_of(msg, len, &m.views[VIEW_BYTES * (size_t)i]);
          body_of(msg, len, &m.view_body[at]);
          m.view_used[i] = used;
          built_in_flight.fetch_add(1);
          __atomic_store_n(&m.view_flags[i], nwc::sq::VIEW_WRITTEN, __ATOMIC_RELEASE);
        }
        // the vote launch: behind it, only for Ok headers that carry a key
        if (key && !again && a.code == 0 && a.kind == nwc::sq::KIND_HEADER && !steer(msg, len, 4)) {
          sig_of(msg, len, key, &m.vote_sigs[64 * (size_t)i]);
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
    g.view_wanted = m.view_wanted.data(); g.views = m.views.data(); g.view_used = m.view_used.data();
    g.view_flags = m.view_flags.data(); g.view_body = m.view_body.data();
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
  // a request that asks for a view is decided by view_alone: never by redo or bypass as well
  int redo(const uint8_t* msg, size_t len, uint64_t, const uint8_t*, uint8_t* digest32, uint8_t* kind) override {
    redo_calls.fetch_add(1);
    CHECK(steer(msg, len, 2) || steer(msg, len, 3));
    CHECK(!asks_view(msg, len));
    return decide(msg, len, digest32, kind);
  }
  int bypass(const uint8_t* msg, size_t len, uint64_t, const uint8_t*, uint8_t* digest32, uint8_t* kind) override {
    bypasses.fetch_add(1);
    CHECK(!asks_view(msg, len));
    return decide(msg, len, digest32, kind);
  }
  int vote_alone(const uint8_t* msg, size_t len, const uint8_t* id32, uint64_t vote_key, uint8_t* sig64) override {
    vote_alone_calls.fetch_add(1);
    const Answer a = answer_of(msg, len);
    CHECK(a.code == 0 && a.kind == nwc::sq::KIND_HEADER);
    CHECK(vote_key != 0 && vote_key == key_of(msg, len));
    CHECK(std::memcmp(id32, a.digest, 32) == 0);
    CHECK(len > byte_cap || steer(msg, len, 2) || steer(msg, len, 3) || steer(msg, len, 4) || (len > 6 && msg[6] == 0xD1));
    sig_of(msg, len, vote_key, sig64);
    return 0;
  }
  int view_alone(const uint8_t* msg, size_t len, uint64_t gc_round, const uint8_t*, uint8_t* digest32, uint8_t* kind,
                 const ViewReq& out) override {
    view_alone_calls.fetch_add(1);
    CHECK(asks_view(msg, len) && gc_round == 5);
    CHECK(len > byte_cap || steer(msg, len, 2) || steer(msg, len, 3) || steer(msg, len, 8) || (len > 6 && msg[6] == 0xD1));
    CHECK(out.rec && out.body && out.body_used && out.body_cap >= nwc::sq::view_body_bound(len));
    record_of(msg, len, out.rec);
    body_of(msg, len, out.body);
    *out.body_used = body_len_of(msg, len);
    return decide(msg, len, digest32, kind);
  }
};

struct Request {
  std::vector<uint8_t> msg;
  uint64_t key;
  bool view;
};
Request make_request(std::mt19937& rng, size_t len, bool ask_view, bool ask_vote, int steer_one_in) {
  Request r;
  r.msg.resize(len);
  for (uint8_t& x : r.msg) x = (uint8_t)rng();
  if (len > 0) r.msg[0] = rng() % 3 ? 0 : (uint8_t)(rng() % 12);   // mostly Ok
  if (len > 1) r.msg[1] = rng() % 3 ? 0 : (uint8_t)(rng() % 4);    // mostly headers
  for (size_t k = 2; k <= 4 && k < len; ++k) r.msg[k] = steer_one_in && rng() % steer_one_in == 0;
  if (len > 5) r.msg[5] = ask_vote ? (uint8_t)(1 + rng() % 3) : 0;
  if (len > 6) r.msg[6] = 0;
  if (len > 7) r.msg[7] = ask_view ? 1 : 0;
  if (len > 8) r.msg[8] = steer_one_in && rng() % steer_one_in == 0;
  r.key = key_of(r.msg.data(), len);
  r.view = asks_view(r.msg.data(), len);
  return r;
}
// What the caller must see; returns rc.
int submit_checked(nwc::sq::Queue& q, const Request& r, bool* voted_out, bool direct = false) {
  uint8_t digest[32], kind = 0xEE, sig[65], rec[VIEW_BYTES + 1];
  int voted = 77;
  uint64_t used = 0xEEEEEEEEull;
  std::memset(digest, 0xEE, sizeof digest);
  std::memset(sig, 0xEE, sizeof sig);
  std::memset(rec, 0xEE, sizeof rec);
  const uint8_t* p = r.msg.data();
  const size_t len = r.msg.size();
  const uint64_t cap = nwc::sq::view_body_bound(len);
  std::vector<uint8_t> body(cap + 1, 0xEE);   // exactly the bound: the address sanitizer watches what lies behind it
  const ViewReq vr{rec, body.data(), cap, &used};
  const int rc = q.submit(p, len, 5, nullptr, digest, &kind, direct, r.key, r.key ? sig : nullptr, r.key ? &voted : nullptr,
                          r.view ? &vr : nullptr);
  const Answer a = answer_of(p, len);
  static const uint8_t zero[VIEW_BYTES] = {0};
  *voted_out = false;
  if (!r.key) {
    CHECK(voted == 77 && sig[0] == 0xEE);   // outputs it did not pass are not touched
  } else {
    CHECK(sig[64] == 0xEE);
    const bool expect = rc >= 0 && a.code == 0 && a.kind == nwc::sq::KIND_HEADER;
    CHECK(voted == (expect ? 1 : 0));
    if (expect) {
      uint8_t want[64];
      sig_of(p, len, r.key, want);
      CHECK(std::memcmp(sig, want, 64) == 0);
    } else {
      CHECK(std::memcmp(sig, zero, 64) == 0);
    }
    *voted_out = voted == 1;
  }
  CHECK(rec[VIEW_BYTES] == 0xEE && body[cap] == 0xEE);
  if (!r.view) {
    CHECK(rec[0] == 0xEE && used == 0xEEEEEEEEull && body[0] == 0xEE);   // a view iff it was asked for
  } else if (rc < 0) {
    CHECK(std::memcmp(rec, zero, VIEW_BYTES) == 0 && used == 0);   // an error: a zeroed record
  } else {
    // its own: this message's record, body length and body, whatever the code
    uint8_t want[VIEW_BYTES];
    record_of(p, len, want);
    CHECK(std::memcmp(rec, want, VIEW_BYTES) == 0);
    CHECK(used == body_len_of(p, len));
    std::vector<uint8_t> wb(cap);
    body_of(p, len, wb.data());
    CHECK(used <= cap && std::memcmp(body.data(), wb.data(), (size_t)std::min<uint64_t>(used, cap)) == 0);
  }
  if (rc < 0) {
    CHECK(digest[0] == 0xEE && kind == 0xEE);
    return rc;
  }
  CHECK(rc == a.code && std::memcmp(digest, a.digest, 32) == 0 && kind == a.kind);
  return rc;
}

// 8 threads x per_thread requests, half of them asking for a view, a quarter also for a vote
void stress(uint32_t max_messages, uint32_t max_wait_us, int per_thread, long fail_group) {
  constexpr uint32_t MSG_CAP = 64;
  constexpr uint64_t BYTE_CAP = 16 << 10;
  constexpr int THREADS = 8;
  FakeBackend be(max_messages ? max_messages : MSG_CAP, BYTE_CAP, fail_group, 60);
  nwc::sq::Queue q(be, FakeBackend::NBUF, max_messages, MSG_CAP, BYTE_CAP, max_wait_us, std::chrono::milliseconds(20));
  std::atomic<uint64_t> answered{0}, errors{0}, views{0}, expect_alone{0}, oversized_viewed{0}, plain_outside{0}, plain_bypassed{0};
  std::vector<std::thread> ts;
  for (int t = 0; t < THREADS; ++t) {
    ts.emplace_back([&, t] {
      std::mt19937 rng(7000 + t);
      for (int k = 0; k < per_thread; ++k) {
        size_t len = 9 + rng() % 3000;
        if (k % 97 == 5) len = rng() % 8;          // too short to ask, the empty message among them
        if (k % 211 == 7 || k % 211 == 8) len = BYTE_CAP + 1 + rng() % 100;   // (one odd k, one even)
        Request r = make_request(rng, len, (k & 1) != 0, (k & 3) == 3, 60);
        auto set = [&](int code, int kind, int again, int unwritten, int unsigned_, int noview) {
          r.msg[0] = (uint8_t)code; r.msg[1] = (uint8_t)kind; r.msg[2] = (uint8_t)again; r.msg[3] = (uint8_t)unwritten;
          r.msg[4] = (uint8_t)unsigned_; r.msg[8] = (uint8_t)noview;
        };
        if (len <= BYTE_CAP && len > 8) {
          if (t == 0 && k == 1) set(0, 0, 0, 0, 0, 1);   // one unwritten view flag early
          if (t == 1 && k == 1) set(0, 0, 0, 1, 0, 0);   // one unwritten word
          if (t == 2 && k == 1) set(0, 0, 1, 0, 0, 0);   // one redo word
          if (t == 3 && k == 3) set(0, 0, 0, 0, 1, 1);   // view and vote both undelivered
          if (t == 4 && k == 1) set(3, 2, 0, 0, 0, 1);   // a refused certificate still gets its record
        }
        bool voted = false;
        const int rc = submit_checked(q, r, &voted);
        answered.fetch_add(1);
        const uint8_t* p = r.msg.data();
        if (rc < 0) {
          CHECK(rc == NWC_ERR_DEVICE && !voted && len <= BYTE_CAP);   // a failed launch: the error, no vote, no view
          errors.fetch_add(1);
          continue;
        }
        const bool outside = steer(p, len, 2) || steer(p, len, 3);
        if (!r.view) {
          if (len > BYTE_CAP) plain_bypassed.fetch_add(1);
          else if (outside) plain_outside.fetch_add(1);
          continue;
        }
        views.fetch_add(1);
        if (len > BYTE_CAP) { oversized_viewed.fetch_add(1); expect_alone.fetch_add(1); }
        else if (outside || steer(p, len, 8)) expect_alone.fetch_add(1);
      }
    });
  }
  for (std::thread& t : ts) t.join();
  const nwc::sq::Stats st = q.stats();
  CHECK(answered.load() == (uint64_t)THREADS * per_thread);
  CHECK(views.load() > 0 && expect_alone.load() > 0 && oversized_viewed.load() > 0);
  // unwritten flags, redo words, unwritten words and oversized messages reached view_alone exactly
  // once each, and redo / bypass saw only the requests without a view
  CHECK(be.view_alone_calls.load() == expect_alone.load() && st.views_alone == expect_alone.load());
  CHECK(st.views_in_flight == views.load() - expect_alone.load());
  CHECK(be.built_in_flight.load() >= st.views_in_flight);   // (a failed vote fallback cannot occur here: equal but for none)
  CHECK(be.redo_calls.load() == plain_outside.load() && be.bypasses.load() == plain_bypassed.load());
  CHECK(be.unwanted_after_wanted.load() > 0);   // buffer reuse after a viewing group was exercised
  if (fail_group >= 0) CHECK(errors.load() == be.failed_messages.load() && errors.load() >= 1);
  else CHECK(errors.load() == 0);
  std::printf("stress max_messages=%u max_wait_us=%u: %llu groups, %llu messages, %llu views in flight, %llu alone, %llu errors\n",
              max_messages, max_wait_us, (unsigned long long)st.groups, (unsigned long long)st.messages,
              (unsigned long long)st.views_in_flight, (unsigned long long)st.views_alone, (unsigned long long)errors.load());
}

// a viewing group of 8 fills a buffer; the groups after it on the same buffers ask for nothing and
// must present a wanted byte of 0 in every slot
void stale_wanted() {
  FakeBackend be(8, 64 << 10, -1, 0);
  nwc::sq::Queue q(be, FakeBackend::NBUF, 8, 8, 64 << 10, 30u * 1000 * 1000);
  for (int round = 0; round < 6; ++round) {
    const bool ask = round % 3 == 0;
    std::vector<std::thread> ts;
    for (int t = 0; t < 8; ++t) {
      ts.emplace_back([&, t] {
        std::mt19937 rng(50 + 8 * round + t);
        Request r = make_request(rng, 40 + 13 * t, ask, false, 0);
        bool voted = false;
        CHECK(submit_checked(q, r, &voted) >= 0 && !voted);
      });
    }
    for (std::thread& t : ts) t.join();
  }
  const nwc::sq::Stats st = q.stats();
  CHECK(st.groups == 6 && st.views_in_flight == 16 && st.views_alone == 0);
  CHECK(be.wanted_slots.load() == 16 && be.unwanted_after_wanted.load() >= 8);
  // `direct` goes round the groups: view_alone decides, bypass is not called; the vote follows
  std::mt19937 rng(9);
  Request d = make_request(rng, 100, true, true, 0);
  d.msg[0] = 0; d.msg[1] = 0; d.msg[6] = 0xD1;
  bool voted = false;
  CHECK(submit_checked(q, d, &voted, true) == 0 && voted);
  d.msg[0] = 1;   // an invalid signature: its record all the same, no vote
  CHECK(submit_checked(q, d, &voted, true) == 1 && !voted);
  CHECK(q.stats().views_alone == 2 && be.view_alone_calls.load() == 2 && be.bypasses.load() == 0 && be.vote_alone_calls.load() == 1);
  // a view with a missing output or too small a body is refused before anything is queued
  const nwc::sq::Stats s0 = q.stats();
  uint8_t rec[VIEW_BYTES], body[256];
  uint64_t used = 9;
  std::memset(rec, 0xEE, sizeof rec);
  const ViewReq small{rec, body, nwc::sq::view_body_bound(100) - 1, &used};
  CHECK(q.submit(d.msg.data(), 100, 5, nullptr, nullptr, nullptr, false, 0, nullptr, nullptr, &small) == NWC_ERR_ARG);
  CHECK(used == 0 && rec[0] == 0 && rec[VIEW_BYTES - 1] == 0);
  const ViewReq nobody{rec, nullptr, 1000, &used};
  CHECK(q.submit(d.msg.data(), 100, 5, nullptr, nullptr, nullptr, false, 0, nullptr, nullptr, &nobody) == NWC_ERR_ARG);
  const ViewReq noused{rec, body, 1000, nullptr};
  CHECK(q.submit(d.msg.data(), 100, 5, nullptr, nullptr, nullptr, false, 0, nullptr, nullptr, &noused) == NWC_ERR_ARG);
  const nwc::sq::Stats s1 = q.stats();
  CHECK(s1.messages == s0.messages && s1.bypassed_messages == s0.bypassed_messages && s1.views_alone == s0.views_alone);
}

// a backend without views (the default view_alone, no view members in its buffers): a request that
// asks gets the error and a zeroed record; one that does not is served as before
void backend_without_views() {
  struct NoViews : FakeBackend {
    using FakeBackend::FakeBackend;
    GroupBuf buffer(int b) override {
      GroupBuf g = FakeBackend::buffer(b);
      g.view_wanted = nullptr; g.views = nullptr; g.view_used = nullptr; g.view_flags = nullptr; g.view_body = nullptr;
      return g;
    }
    int view_alone(const uint8_t* a, size_t b, uint64_t c, const uint8_t* d, uint8_t* e, uint8_t* f, const ViewReq& g) override {
      return nwc::sq::Backend::view_alone(a, b, c, d, e, f, g);
    }
  } be(8, 4096, -1, 0);
  nwc::sq::Queue q(be, FakeBackend::NBUF, 0, 8, 4096, 0, std::chrono::milliseconds(5));
  std::mt19937 rng(3);
  Request r = make_request(rng, 64, false, false, 0);
  r.msg[7] = 1;   // the caller asks; the fake device's check of the wanted byte is moot (it reads its own array)
  r.view = true;
  uint8_t dig[32], kind = 0xEE, rec[VIEW_BYTES], body[128];
  uint64_t used = 7;
  std::memset(dig, 0xEE, 32);
  std::memset(rec, 0xEE, sizeof rec);
  const ViewReq vr{rec, body, sizeof body, &used};
  for (FakeBackend::Mem& m : be.mem) {   // what a member would have written, had the buffers view members
    std::fill(m.view_wanted.begin(), m.view_wanted.end(), 1);
    std::fill(m.view_flags.begin(), m.view_flags.end(), 0);
  }
  CHECK(q.submit(r.msg.data(), r.msg.size(), 5, nullptr, dig, &kind, false, 0, nullptr, nullptr, &vr) == NWC_ERR_ARG);
  static const uint8_t zero[VIEW_BYTES] = {0};
  CHECK(used == 0 && std::memcmp(rec, zero, VIEW_BYTES) == 0 && kind == 0xEE && dig[0] == 0xEE);
}

// stop() with viewers blocked in a group that waits for company: launched at once, every viewer
// gets its view and has left when stop returns
void stop_with_blocked_viewers() {
  FakeBackend be(64, 64 << 10, -1, 0);
  nwc::sq::Queue q(be, FakeBackend::NBUF, 64, 64, 64 << 10, 30u * 1000 * 1000);
  std::atomic<int> left{0};
  std::vector<std::thread> ts;
  for (int t = 0; t < 4; ++t) {
    ts.emplace_back([&, t] {
      std::mt19937 rng(90 + t);
      Request r = make_request(rng, 500, true, t == 0, 0);
      r.msg[0] = 0;
      r.msg[1] = 0;
      bool voted = false;
      CHECK(submit_checked(q, r, &voted) == 0 && voted == (t == 0));
      left.fetch_add(1);
    });
  }
  while (q.stats().messages < 4) std::this_thread::yield();
  const auto t0 = std::chrono::steady_clock::now();
  q.stop();
  CHECK(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(10));
  for (std::thread& t : ts) t.join();
  CHECK(left.load() == 4 && q.stats().groups == 1 && q.stats().views_in_flight == 4 && q.stats().votes_in_flight == 1);
  uint8_t msg[16] = {0}, rec[VIEW_BYTES], body[80];
  uint64_t used = 9;
  std::memset(rec, 0xEE, sizeof rec);
  const ViewReq vr{rec, body, sizeof body, &used};
  CHECK(q.submit(msg, 16, 5, nullptr, nullptr, nullptr, false, 0, nullptr, nullptr, &vr) == NWC_ERR_NOT_INIT && used == 0 && rec[0] == 0);
}

}  // namespace

int main(int argc, char** argv) {
  const int per_thread = argc > 1 ? std::atoi(argv[1]) : 2000;
  stress(16, 0, per_thread, 37);
  stress(0, 150, per_thread, -1);
  stale_wanted();
  backend_without_views();
  stop_with_blocked_viewers();
  if (g_failures.load()) {
    std::fprintf(stderr, "%llu checks failed\n", (unsigned long long)g_failures.load());
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
