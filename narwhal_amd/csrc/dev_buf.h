// Ownership of device and pinned host buffers: one handle type (Buf) and the set that owns every
// handle of a device context (BufSet).  Nothing of the GPU runtime is named here: the includer
// supplies the allocator A (nwc_api.hip: the runtime's calls; tests/cpp/dev_buf_host.cpp: a
// counting fake),
//   A::Error, A::ok, A::Stream
//   A::alloc(void**, bytes)                 A::free(void*)
//   A::alloc_async(void**, bytes, stream)   A::free_async(void*, stream)
//   A::alloc_pinned(void** host, void** dev, bytes)   A::free_pinned(void* host)
// so the rules below run on the CPU under the host sanitizers.
//
//  - Only release() / release_async() (and what calls them: alloc over a held block, ensure, adopt,
//    the set's release_*) free.  No destructor calls the allocator: a process may leave without
//    nwc_shutdown, and static destructors then run after the runtime is gone.  A handle that goes
//    away forgets its block.
//  - A release clears the pointer and the size before it reports the free's result: a failed free
//    never leaves a stale pointer behind.  Releasing an empty handle does nothing.
//  - alloc over a held block releases it first, so a sequence of allocs is safe to run again.
//  - bytes() is the size asked of the allocator, not what it rounded to.
//  - A block is freed stream-ordered only if it was allocated stream-ordered; release_async of a
//    plain block is a plain free (the block is in no stream's pool; the plain free waits for the
//    device itself), and release() of a stream-ordered block is a plain free (valid once the device
//    has passed its users).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace nwc::buf {

enum class Kind : uint8_t { Device, DeviceAsync, Pinned };
// where nwc_memory_info reports a buffer's bytes (Uncounted: nowhere)
enum class Account : uint8_t { Tables, Committee, AutoCache, Scratch, Uncounted };
enum Trim : bool { Keep = false, Trimmable = true };   // whether nwc_trim drops the buffer
constexpr size_t NO_SHRINK = ~(size_t)0;                // ensure's keep: grow only

template <class A> class BufSet;

// The untyped handle: what the set and the growth policy work on.
template <class A>
class RawBuf {
 public:
  using Error = typename A::Error;
  using Stream = typename A::Stream;

  RawBuf() = default;   // detached: in no set (a local that adopt() hands to a member)
  RawBuf(BufSet<A>& set, Account account, Trim trim, Kind kind = Kind::Device)
      : set_(&set), account_(account), trim_(trim), kind_(kind) {
    set.bufs_.push_back(this);
  }
  RawBuf(RawBuf&& o) noexcept : set_(o.set_), account_(o.account_), trim_(o.trim_) {
    if (set_) set_->bufs_.push_back(this);
    take(o);
  }
  RawBuf(const RawBuf&) = delete;
  RawBuf& operator=(const RawBuf&) = delete;
  RawBuf& operator=(RawBuf&&) = delete;   // adopt(): it may have to free, and reports that
  ~RawBuf() {
    if (set_) set_->bufs_.erase(std::find(set_->bufs_.begin(), set_->bufs_.end(), this));
  }

  size_t bytes() const { return bytes_; }
  Kind kind() const { return kind_; }
  Account account() const { return account_; }
  bool trimmable() const { return trim_; }
  void* raw() const { return p_; }

  // A plain block of `bytes` (a handle constructed Kind::Pinned: pinned host memory and its device alias).
  Error alloc(size_t bytes) {
    if (Error e = release(); e != A::ok) return e;
    const bool pinned = kind_ == Kind::Pinned;
    if (Error e = pinned ? A::alloc_pinned(&p_, &dev_, bytes) : A::alloc(&p_, bytes); e != A::ok) {
      p_ = dev_ = nullptr;   // (an allocator that fails holds nothing)
      return e;
    }
    if (!pinned) kind_ = Kind::Device;
    bytes_ = bytes;
    return A::ok;
  }
  // A stream-ordered block of `bytes` from s's pool.
  Error alloc_async(size_t bytes, Stream s) {
    if (Error e = release(); e != A::ok) return e;
    if (Error e = A::alloc_async(&p_, bytes, s); e != A::ok) {
      p_ = nullptr;
      return e;
    }
    kind_ = Kind::DeviceAsync;
    bytes_ = bytes;
    return A::ok;
  }
  Error release() {
    void* const p = forget();
    if (!p) return A::ok;
    return kind_ == Kind::Pinned ? A::free_pinned(p) : A::free(p);
  }
  // Behind the work queued on s, if the block came from a stream's pool.
  Error release_async(Stream s) {
    if (kind_ != Kind::DeviceAsync) return release();
    void* const p = forget();
    return p ? A::free_async(p, s) : A::ok;
  }
  // Takes o's block (o is left empty) after releasing the one held; keeps this handle's own set,
  // account and trim flag.
  Error adopt(RawBuf&& o) {
    const Error e = release();
    take(o);
    return e;
  }

  // Whether a block that serves `need` bytes is held and ensure(need, .., keep) would leave it:
  // large enough, and not a block above `keep` bytes of which under a quarter is needed.
  bool fits(size_t need, size_t keep = NO_SHRINK) const { return need <= bytes_ && !(bytes_ > keep && need < bytes_ / 4); }
  // Replaces the block by one of need + headroom bytes unless it fits.  keep = NO_SHRINK only
  // grows.  The caller has made sure that nothing on the device still uses the old block.
  Error ensure(size_t need, size_t headroom = 0, size_t keep = NO_SHRINK) {
    if (fits(need, keep)) return A::ok;
    return alloc(need + headroom);
  }

 protected:
  void* p_ = nullptr;
  void* dev_ = nullptr;   // Pinned: the device's address of the block

 private:
  friend class BufSet<A>;
  void* forget() {
    void* const p = p_;
    p_ = dev_ = nullptr;
    bytes_ = 0;
    return p;
  }
  void take(RawBuf& o) {
    p_ = o.p_;
    dev_ = o.dev_;
    bytes_ = o.bytes_;
    kind_ = o.kind_;
    o.forget();
  }
  size_t bytes_ = 0;
  BufSet<A>* set_ = nullptr;
  Account account_ = Account::Uncounted;
  Trim trim_ = Keep;
  Kind kind_ = Kind::Device;
};

template <class T, class A>
class Buf : public RawBuf<A> {
 public:
  using RawBuf<A>::RawBuf;
  T* get() const { return static_cast<T*>(this->p_); }
  T* dev() const { return static_cast<T*>(this->dev_); }   // Pinned: the device alias
  operator T*() const { return get(); }                    // reads like the pointer it owns
};

// Every buffer of one device context.  Handles register themselves on construction and leave on
// destruction, so the set must outlive them (declare it before them).
template <class A>
class BufSet {
 public:
  using Error = typename A::Error;
  BufSet() = default;
  BufSet(const BufSet&) = delete;
  BufSet& operator=(const BufSet&) = delete;

  // Plain frees of everything held (the device has passed every user); the first error, after
  // every buffer has been released.
  Error release_all() { return release_if([](const RawBuf<A>&) { return true; }); }
  Error release_trimmable() { return release_if([](const RawBuf<A>& b) { return b.trimmable(); }); }
  size_t bytes(Account a) const {
    size_t sum = 0;
    for (const RawBuf<A>* b : bufs_)
      if (b->account() == a) sum += b->bytes();
    return sum;
  }
  size_t size() const { return bufs_.size(); }

 private:
  friend class RawBuf<A>;
  template <class F>
  Error release_if(F pick) {
    Error first = A::ok;
    for (RawBuf<A>* b : bufs_) {
      if (!pick(*b)) continue;
      const Error e = b->release();
      if (first == A::ok) first = e;
    }
    return first;
  }
  std::vector<RawBuf<A>*> bufs_;
};

}  // namespace nwc::buf
