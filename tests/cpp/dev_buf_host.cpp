// Drives narwhal_amd/csrc/dev_buf.h against a counting fake allocator, on the CPU.  Built by
// tests/test_dev_buf_host.py with the address and undefined-behaviour sanitizers and run as a child
// process.  Exit status 0 and a last line "ok" mean every check held.
//
// The fake hands out malloc blocks and records every alloc and free with its kind; it can fail the
// k-th allocation and make frees report an error (the block still goes back, as a real failed free
// leaves nothing to retry with).  The rule it checks on every free, the one dev_buf.h states and
// nwc_shutdown relies on: a block is freed by the call of its own kind, or -- a stream-ordered
// block only -- by the plain free.  A stream-ordered free of a plain block, a free of a pointer
// that is not live (a second free) and a device free of pinned memory are violations.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <map>
#include <utility>
#include <vector>

#include "dev_buf.h"

namespace {

using nwc::buf::Account;
using nwc::buf::Keep;
using nwc::buf::Kind;
using nwc::buf::NO_SHRINK;
using nwc::buf::Trimmable;

int g_failures = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++g_failures;                                                                 \
    }                                                                               \
  } while (0)

struct Fake {
  using Error = int;
  using Stream = int;   // streams are numbers; 0 = none
  static constexpr Error ok = 0;
  static constexpr Error oom = 2, bad_free = 17;

  struct Block { Kind kind; size_t bytes; };
  static inline std::map<void*, Block> live;
  static inline long allocs = 0, frees = 0, async_frees = 0, violations = 0;
  static inline long fail_alloc = 0;   // fail when `allocs` reaches this count (0 = never)
  static inline bool fail_frees = false;
  static inline std::vector<int> free_streams;   // the stream of every stream-ordered free

  static void reset() {
    reclaim();
    allocs = frees = async_frees = violations = 0;
    fail_alloc = 0;
    fail_frees = false;
    free_streams.clear();
  }
  // blocks that handles forgot on purpose: back to malloc without counting
  static void reclaim() {
    for (auto& kv : live) std::free(kv.first);
    live.clear();
  }
  static size_t live_bytes() {
    size_t s = 0;
    for (auto& kv : live) s += kv.second.bytes;
    return s;
  }
  static Error get(void** p, size_t bytes, Kind kind) {
    if (++allocs == fail_alloc) return oom;
    *p = std::malloc(bytes ? bytes : 1);
    live[*p] = Block{kind, bytes};
    return ok;
  }
  static Error put(void* p, bool kind_ok) {
    ++frees;
    auto it = live.find(p);
    if (it == live.end() || !kind_ok) {
      ++violations;
      if (it == live.end()) return bad_free;
    }
    live.erase(it);
    std::free(p);
    return fail_frees ? bad_free : ok;
  }
  static Kind kind_of(void* p) {
    auto it = live.find(p);
    return it == live.end() ? Kind::Device : it->second.kind;
  }
  static Error alloc(void** p, size_t bytes) { return get(p, bytes, Kind::Device); }
  static Error alloc_async(void** p, size_t bytes, Stream) { return get(p, bytes, Kind::DeviceAsync); }
  static Error alloc_pinned(void** host, void** dev, size_t bytes) {
    const Error e = get(host, bytes, Kind::Pinned);
    if (e == ok) *dev = *host;
    return e;
  }
  static Error free(void* p) { return put(p, kind_of(p) != Kind::Pinned); }
  static Error free_async(void* p, Stream s) {
    ++async_frees;
    free_streams.push_back(s);
    return put(p, kind_of(p) == Kind::DeviceAsync);
  }
  static Error free_pinned(void* p) { return put(p, kind_of(p) == Kind::Pinned); }
};

template <class T> using Buf = nwc::buf::Buf<T, Fake>;
using RawBuf = nwc::buf::RawBuf<Fake>;
using BufSet = nwc::buf::BufSet<Fake>;

// bytes(account) of the set against what the allocator was asked for on behalf of these handles
void check_accounts(const BufSet& set, std::initializer_list<const RawBuf*> bufs) {
  size_t want[5] = {0, 0, 0, 0, 0};
  for (const RawBuf* b : bufs) {
    if (!b->raw()) {
      CHECK(b->bytes() == 0);
      continue;
    }
    auto it = Fake::live.find(b->raw());
    CHECK(it != Fake::live.end());
    if (it == Fake::live.end()) continue;
    CHECK(it->second.bytes == b->bytes());
    want[(int)b->account()] += it->second.bytes;
  }
  for (Account a : {Account::Tables, Account::Committee, Account::AutoCache, Account::Scratch, Account::Uncounted})
    CHECK(set.bytes(a) == want[(int)a]);
}

void test_release() {
  Fake::reset();
  BufSet set;
  Buf<uint32_t> a(set, Account::Scratch, Trimmable);
  Buf<uint8_t> pin(set, Account::Uncounted, Keep, Kind::Pinned);
  CHECK(a.get() == nullptr && a.bytes() == 0 && !a);
  CHECK(a.release() == Fake::ok && a.release_async(3) == Fake::ok && Fake::frees == 0);   // empty: no call
  CHECK(a.alloc(1001) == Fake::ok && a.get() && a.bytes() == 1001 && a.kind() == Kind::Device);   // as asked, not rounded
  uint32_t* const first = a.get();
  CHECK(a.alloc(40) == Fake::ok && Fake::frees == 1 && Fake::live.count(first) == 0 && a.bytes() == 40);   // released first
  CHECK(a.release() == Fake::ok && Fake::frees == 2 && !a.get() && a.bytes() == 0);
  CHECK(a.release() == Fake::ok && Fake::frees == 2);   // release after release: zero calls
  // a free that reports an error still leaves the handle empty, and is not tried again
  CHECK(a.alloc(64) == Fake::ok);
  Fake::fail_frees = true;
  CHECK(a.release() == Fake::bad_free && !a.get() && a.bytes() == 0 && set.bytes(Account::Scratch) == 0);
  CHECK(a.release() == Fake::ok && Fake::frees == 3);
  CHECK(a.alloc_async(64, 1) == Fake::ok);
  CHECK(a.release_async(1) == Fake::bad_free && !a.get() && a.bytes() == 0);
  Fake::fail_frees = false;
  // a failed alloc holds nothing
  Fake::fail_alloc = Fake::allocs + 1;
  CHECK(a.alloc(8) == Fake::oom && !a.get() && a.bytes() == 0);
  // kinds: stream-ordered blocks go back stream-ordered on the stream given, or by the plain free;
  // release_async of a plain block is a plain free; pinned memory has its own pair and an alias
  CHECK(a.alloc_async(256, 7) == Fake::ok && a.kind() == Kind::DeviceAsync);
  CHECK(a.release_async(9) == Fake::ok && Fake::async_frees == 2 && Fake::free_streams.back() == 9);
  CHECK(a.alloc_async(256, 7) == Fake::ok && a.release() == Fake::ok && Fake::async_frees == 2);
  CHECK(a.alloc(256) == Fake::ok && a.release_async(9) == Fake::ok && Fake::async_frees == 2);
  CHECK(pin.alloc(4) == Fake::ok && pin.kind() == Kind::Pinned && pin.dev() == pin.get() && pin.dev());
  CHECK(pin.release_async(2) == Fake::ok && !pin.get() && !pin.dev() && Fake::async_frees == 2);
  CHECK(Fake::violations == 0 && Fake::live.empty());
  // moves: the new handle joins the old one's set and account; adopt keeps the target's own
  CHECK(a.alloc(100) == Fake::ok);
  {
    Buf<uint32_t> moved(std::move(a));
    CHECK(!a.get() && a.bytes() == 0 && moved.bytes() == 100 && set.size() == 3 && set.bytes(Account::Scratch) == 100);
    Buf<uint32_t> loose;   // detached
    CHECK(loose.alloc_async(300, 4) == Fake::ok && set.bytes(Account::Scratch) == 100);
    CHECK(moved.adopt(std::move(loose)) == Fake::ok && !loose.get() && moved.bytes() == 300 && moved.kind() == Kind::DeviceAsync);
    CHECK(set.bytes(Account::Scratch) == 300 && Fake::live.size() == 1);
    // no destructor frees: the handle leaves the set and forgets its block
    const long frees = Fake::frees;
    { Buf<uint32_t> gone(std::move(moved)); }
    CHECK(Fake::frees == frees && Fake::live.size() == 1);
  }
  CHECK(set.size() == 2 && set.bytes(Account::Scratch) == 0 && set.release_all() == Fake::ok && Fake::live.size() == 1);
  Fake::reclaim();
  CHECK(Fake::violations == 0);
  std::puts("release");
}

// the shape of a device context: some buffers per account, some trimmable
struct Ctx {
  BufSet set;
  Buf<uint8_t> table_a{set, Account::Tables, Keep}, table_b{set, Account::Tables, Keep};
  Buf<uint8_t> cm{set, Account::Committee, Keep};
  Buf<uint8_t> cache{set, Account::AutoCache, Keep}, lk{set, Account::AutoCache, Trimmable};
  Buf<uint8_t> scratch{set, Account::Scratch, Trimmable}, arena{set, Account::Scratch, Trimmable};
  Buf<uint8_t> counter{set, Account::Uncounted, Keep};
  Buf<uint8_t> pinned{set, Account::Uncounted, Keep, Kind::Pinned};
};

void test_accounts_and_trim() {
  Fake::reset();
  {
    Ctx c;
    auto step = [&] { check_accounts(c.set, {&c.table_a, &c.table_b, &c.cm, &c.cache, &c.lk, &c.scratch, &c.arena, &c.counter, &c.pinned}); };
    step();
    CHECK(c.table_a.alloc(2 * 129 * 160) == Fake::ok); step();
    CHECK(c.table_b.alloc(3) == Fake::ok); step();
    CHECK(c.cm.alloc(36 * 5) == Fake::ok); step();
    CHECK(c.cache.alloc_async(1 << 12, 1) == Fake::ok); step();
    CHECK(c.lk.alloc(16) == Fake::ok); step();
    CHECK(c.scratch.alloc(12345) == Fake::ok); step();
    CHECK(c.arena.ensure(1000, 1000 / 4 + (1 << 20)) == Fake::ok); step();
    CHECK(c.counter.alloc(4) == Fake::ok && c.pinned.alloc(1 << 20) == Fake::ok); step();
    CHECK(c.set.bytes(Account::Tables) == 2 * 129 * 160 + 3 && c.set.bytes(Account::Scratch) == 12345 + 1000 + 250 + (1 << 20));
    CHECK(c.scratch.alloc(777) == Fake::ok); step();   // replaced: the old size is gone from the sum
    CHECK(c.cache.release_async(1) == Fake::ok); step();
    CHECK(c.cache.alloc(99) == Fake::ok); step();
    std::puts("accounts");
    // release_trimmable: the flagged buffers and only those
    const size_t tables = c.set.bytes(Account::Tables), cmb = c.set.bytes(Account::Committee);
    const long frees = Fake::frees;
    CHECK(c.set.release_trimmable() == Fake::ok); step();
    CHECK(Fake::frees == frees + 3 && !c.lk.get() && !c.scratch.get() && !c.arena.get());
    CHECK(c.table_a.get() && c.table_b.get() && c.cm.get() && c.cache.get() && c.counter.get() && c.pinned.get());
    CHECK(c.set.bytes(Account::Scratch) == 0 && c.set.bytes(Account::AutoCache) == 99 && c.set.bytes(Account::Tables) == tables &&
          c.set.bytes(Account::Committee) == cmb);
    CHECK(c.set.release_trimmable() == Fake::ok && Fake::frees == frees + 3);
    // a failing free: every flagged buffer is still released, the first error comes back
    CHECK(c.scratch.alloc(10) == Fake::ok && c.arena.alloc(10) == Fake::ok);
    Fake::fail_frees = true;
    CHECK(c.set.release_trimmable() == Fake::bad_free && !c.scratch.get() && !c.arena.get() && Fake::frees == frees + 5);
    Fake::fail_frees = false;
    CHECK(c.set.release_all() == Fake::ok); step();
    CHECK(Fake::live.empty() && Fake::frees == Fake::allocs && Fake::violations == 0);   // every block exactly once
    CHECK(c.set.release_all() == Fake::ok && Fake::frees == Fake::allocs);
  }
  std::puts("trim");
}

// ensure_verify_tables' shape: ten buffers allocated in sequence straight into the members, the
// sequence left at the first failure and run again from the top by the next call.
struct Tables {
  BufSet set;
  std::vector<Buf<uint8_t>> bufs;
  Tables() {
    bufs.reserve(10);   // (handles register their address: no reallocation)
    for (int i = 0; i < 10; ++i) bufs.emplace_back(set, i < 8 ? Account::Tables : Account::AutoCache, Keep);
  }
  int build() {
    for (size_t i = 0; i < bufs.size(); ++i)
      if (int e = bufs[i].alloc(100 + 10 * i)) return e;
    return Fake::ok;
  }
};

void test_tables_retry() {
  for (long k = 1; k <= 10; ++k) {
    Fake::reset();
    Tables t;
    Fake::fail_alloc = k;
    CHECK(t.build() == Fake::oom && Fake::live.size() == (size_t)(k - 1));
    CHECK(t.build() == Fake::ok && Fake::live.size() == 10);   // what the failed run left was released on the way
    CHECK(t.set.bytes(Account::Tables) + t.set.bytes(Account::AutoCache) == Fake::live_bytes());
    CHECK(t.set.release_all() == Fake::ok && Fake::live.empty() && Fake::violations == 0 && Fake::frees == Fake::allocs - 1);
  }
  std::puts("tables retry");
}

// auto_grow's shape: four new stream-ordered arrays, the old ones freed behind the copies and
// replaced; a failure gives the new ones back and keeps the old.
struct AutoCache {
  BufSet set;
  Buf<uint8_t> a{set, Account::AutoCache, Keep}, b{set, Account::AutoCache, Keep}, c{set, Account::AutoCache, Keep},
      d{set, Account::AutoCache, Keep};
  int grow(size_t n, int stream) {
    Buf<uint8_t> na, nb, nc, nd;
    const auto get = [&]() -> int {
      if (int e = na.alloc_async(32 * n, stream)) return e;
      if (int e = nb.alloc_async(4 * n, stream)) return e;
      if (int e = nc.alloc_async(129 * n, stream)) return e;
      return nd.alloc_async(1000 * n, stream);
    };
    if (int e = get()) {
      for (RawBuf* x : std::initializer_list<RawBuf*>{&na, &nb, &nc, &nd}) (void)x->release_async(stream);
      return e;
    }
    int freed = Fake::ok;
    const auto swap_in = [&](RawBuf& held, RawBuf& fresh) {
      if (int e = held.release_async(stream); freed == Fake::ok) freed = e;
      (void)held.adopt(std::move(fresh));
    };
    swap_in(a, na); swap_in(b, nb); swap_in(c, nc); swap_in(d, nd);
    return freed;
  }
};

void test_auto_grow_retry() {
  for (long k = 1; k <= 4; ++k) {
    Fake::reset();
    AutoCache ac;
    CHECK(ac.grow(16, 5) == Fake::ok && Fake::live.size() == 4 && Fake::frees == 0);
    const void* const held = ac.a.get();
    Fake::fail_alloc = Fake::allocs + k;
    CHECK(ac.grow(32, 5) == Fake::oom && Fake::live.size() == 4 && ac.a.get() == held);   // the cache keeps its arrays
    CHECK(ac.set.bytes(Account::AutoCache) == 16 * (32 + 4 + 129 + 1000));
    CHECK(ac.grow(32, 5) == Fake::ok && Fake::live.size() == 4 && ac.a.get() != held);
    CHECK(ac.set.bytes(Account::AutoCache) == 32 * (32 + 4 + 129 + 1000) && Fake::live_bytes() == 32 * (32 + 4 + 129 + 1000));
    CHECK(Fake::async_frees == (k - 1) + 4);   // the failed run's new arrays and the old four, all on the stream
    for (int s : Fake::free_streams) CHECK(s == 5);
    CHECK(ac.set.release_all() == Fake::ok && Fake::live.empty() && Fake::violations == 0 && Fake::frees == Fake::allocs - 1);
  }
  std::puts("auto_grow retry");
}

// ensure against worked values of the two policies it replaces:
//   grow only (the arenas): nothing while need <= cap, else a block of need + need / 4 + 1 MiB;
//   grow or shrink (the batch entries' buffers): also replaced by a block of `need` when cap > keep
//   and need < cap / 4.
void test_ensure() {
  Fake::reset();
  BufSet set;
  Buf<uint8_t> arena(set, Account::Scratch, Trimmable);
  const auto arena_ensure = [&](size_t need) { return arena.ensure(need, need / 4 + (1 << 20)); };
  CHECK(arena_ensure(1000) == Fake::ok && arena.bytes() == 1049826 && Fake::allocs == 1);
  CHECK(arena.fits(1049826) && arena_ensure(1049826) == Fake::ok && Fake::allocs == 1);   // need == capacity
  CHECK(arena_ensure(1) == Fake::ok && arena_ensure(0) == Fake::ok && Fake::allocs == 1);   // never shrinks
  CHECK(!arena.fits(1049827) && arena_ensure(1049827) == Fake::ok && Fake::allocs == 2 && Fake::frees == 1);   // one byte over
  CHECK(arena.bytes() == 1049827 + 262456 + 1048576);
  // pinned stage and the pair / sign buffers: grow only, no headroom
  Buf<uint8_t> stage(set, Account::Uncounted, Keep, Kind::Pinned);
  CHECK(stage.ensure(1 << 20) == Fake::ok && stage.bytes() == (1 << 20) && stage.ensure(1 << 20) == Fake::ok && Fake::allocs == 3);
  CHECK(stage.ensure((1 << 20) + 1) == Fake::ok && stage.bytes() == (1 << 20) + 1 && stage.dev() == stage.get());
  // grow or shrink, keep = 4096
  const size_t keep = 4096;
  Buf<uint8_t> b(set, Account::Scratch, Trimmable);
  long n = Fake::allocs;
  CHECK(b.ensure(4096, 0, keep) == Fake::ok && b.bytes() == 4096 && Fake::allocs == ++n);
  CHECK(b.ensure(4096, 0, keep) == Fake::ok && Fake::allocs == n);               // need == capacity
  CHECK(b.ensure(1, 0, keep) == Fake::ok && b.ensure(0, 0, keep) == Fake::ok && Fake::allocs == n);   // at keep: never shrinks
  CHECK(b.ensure(4097, 0, keep) == Fake::ok && b.bytes() == 4097 && Fake::allocs == ++n);   // one byte over: exactly need
  CHECK(b.fits(1024, keep) && b.ensure(1024, 0, keep) == Fake::ok && Fake::allocs == n);    // at a quarter (4097 / 4 = 1024): stays
  CHECK(!b.fits(1023, keep) && b.ensure(1023, 0, keep) == Fake::ok && b.bytes() == 1023 && Fake::allocs == ++n);   // just under: shrinks to need
  CHECK(b.ensure(10, 0, keep) == Fake::ok && b.bytes() == 1023 && Fake::allocs == n);       // below keep again
  CHECK(b.ensure(1 << 20, 0, keep) == Fake::ok && b.ensure((1 << 18) - 1, 0, NO_SHRINK) == Fake::ok && b.bytes() == (1 << 20));
  // a failed replacement leaves the handle empty (the old block went first), and the next call allocates
  Fake::fail_alloc = Fake::allocs + 1;
  CHECK(b.ensure((1 << 20) + 1, 0, keep) == Fake::oom && !b.get() && b.bytes() == 0 && !b.fits(1));
  CHECK(b.fits(0) && b.ensure(5, 0, keep) == Fake::ok && b.bytes() == 5);
  CHECK(set.release_all() == Fake::ok && Fake::live.empty() && Fake::violations == 0);
  std::puts("ensure");
}

}  // namespace

int main() {
  test_release();
  test_accounts_and_trim();
  test_tables_retry();
  test_auto_grow_retry();
  test_ensure();
  if (g_failures) {
    std::fprintf(stderr, "%d checks failed\n", g_failures);
    return 1;
  }
  std::puts("ok");
  return 0;
}
