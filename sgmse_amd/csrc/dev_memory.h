// Owning holders over the drt:: layer (sgmse_devrt.h: the HIP runtime in the product, the CPU emulator in the tests): device and
// page-locked host buffers, events, and the event pair of a timed section.  All move-only; each releases what it holds in its
// destructor, so an exception between an allocation and the end of its scope leaks nothing and leaves no pointer behind.
#pragma once
#include <cstdio>
#include <stdexcept>
#include <string>
#include <utility>
#include <sgmse_devrt.h>

namespace sgmse {

struct EngineError : std::runtime_error { using std::runtime_error::runtime_error; };
// an argument the engine can only judge inside a call (the C boundary reports SGMSE_EINVAL, not SGMSE_ERUNTIME)
struct EngineArgError : EngineError { using EngineError::EngineError; };

#define SG_CHECK(expr) do { int _e = (expr); if (_e != 0) { char _b[256]; snprintf(_b, sizeof _b, "%s failed: %s (%d)", #expr, drt::error_string(_e), _e); throw EngineError(_b); } } while (0)
#define SG_REQUIRE(cond, msg) do { if (!(cond)) throw EngineError(std::string(msg)); } while (0)

// One allocation: device memory (PINNED = false) or page-locked host memory (PINNED = true).
template <bool PINNED>
class Buffer {
 public:
  Buffer() = default;
  Buffer(Buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); cap_ = std::exchange(o.cap_, 0); }
    return *this;
  }
  ~Buffer() { reset(); }
  // (freeing device memory waits for the device: safe also while launches that use the buffer are still queued)
  void reset() {
    if (p_) { if (PINNED) drt::free_host(p_); else drt::free_dev(p_); }
    p_ = nullptr; cap_ = 0;
  }
  // Grow-only: at least `bytes` (and never fewer than 256) afterwards; true if it allocated -- the old contents are gone then.  The
  // holder is empty while it allocates: a failed allocation leaves a null pointer and capacity 0, never the freed block.
  // poison (SGMSE_POISON=1, tests): a fresh device allocation is filled with 0xFF bytes, a NaN in every float, on `stream`.
  bool ensure(size_t bytes, drt::stream_t stream = {}, bool poison = false) {
    if (bytes == 0) bytes = 256;
    if (p_ && bytes <= cap_) return false;
    reset();
    void* p = nullptr;
    if (PINNED) SG_CHECK(drt::malloc_host(&p, bytes));
    else SG_CHECK(drt::malloc_dev(&p, bytes));
    p_ = p; cap_ = bytes;
    if (!PINNED && poison) SG_CHECK(drt::memset_dev(p_, 0xFF, bytes, stream));
    return true;
  }
  // a fresh allocation of `bytes` whatever it held
  void renew(size_t bytes, drt::stream_t stream = {}, bool poison = false) { reset(); ensure(bytes, stream, poison); }
  template <class T = float> T* as() const { return static_cast<T*>(p_); }
  size_t capacity() const { return cap_; }
 private:
  void* p_ = nullptr;
  size_t cap_ = 0;
};
using DevBuf = Buffer<false>;
// ... of elements of one type: reads as the T* it holds (kernel launch arguments take get(): holders are not copied)
template <class T, bool PINNED = false>
struct Array : Buffer<PINNED> {
  T* get() const { return this->template as<T>(); }
  operator T*() const { return get(); }
};
template <class T> using DevArray = Array<T, false>;
template <class T> using PinnedArray = Array<T, true>;

// One event, created on demand (checked), destroyed with its holder.  Order: no timing, for stream_wait_event.
class Event {
 public:
  enum Kind { Timing, Order };
  Event() = default;
  explicit Event(Kind k) { create(k); }
  Event(Event&& o) noexcept : e_(o.e_), live_(std::exchange(o.live_, false)) {}
  Event& operator=(Event&&) = delete;
  ~Event() { if (live_) drt::event_destroy(&e_); }
  void create(Kind k = Timing) {
    if (live_) return;
    if (k == Order) SG_CHECK(drt::event_create_order(&e_)); else SG_CHECK(drt::event_create(&e_));
    live_ = true;
  }
  bool live() const { return live_; }
  drt::event_t* get() { return &e_; }
 private:
  drt::event_t e_{};
  bool live_ = false;
};

// The event pair around a timed section of one stream.
class EventTimer {
 public:
  void start(drt::stream_t stream) { drt::event_record(a_.get(), stream); }
  float stop_ms(drt::stream_t stream) {      // waits for the section to finish
    drt::event_record(b_.get(), stream);
    drt::event_sync(b_.get());
    return drt::event_elapsed_ms(*a_.get(), *b_.get());
  }
 private:
  Event a_{Event::Timing}, b_{Event::Timing};
};

}  // namespace sgmse
