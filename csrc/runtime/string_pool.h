// Recycled request-body buffers for the serving front ends.
//
// A request body is filled on the connection's I/O thread and released on another thread (a decode thread, or a
// proxy worker for the gateway).  Allocated with malloc and freed that way, every request moved a ~100-600 KB
// chunk between glibc arenas: the I/O threads' arenas fragmented and held ~115 MB after a protocol sweep until a
// periodic malloc_trim returned it (round 5).  Here the body's storage goes back to a shared
// free list instead of to the allocator, and the I/O thread's next request reuses its capacity: in steady state
// no body is allocated or freed at all, on any thread.
//
// The pool is bounded in count (`max_keep`) and in the capacity it keeps per string (`max_capacity`): a burst
// beyond it, or one very large upload, is freed normally.
//
// It is also bounded in the bytes it retains.  Strings never shrink, so 1024 kept strings that once held 4.9 MB
// tensor requests would pin 5 GB.  With `set_budget_slots(n)` the pool keeps at most n times the largest capacity
// it has seen (n = the bodies that can be in flight at once: one per I/O thread plus the requests queued behind
// them); a returned string that would take the retained bytes past that is freed instead.  0 slots: no byte budget.
#pragma once

#include <cstddef>
#include <mutex>
#include <string>
#include <vector>

namespace arena {

class StringPool {
 public:
  explicit StringPool(size_t max_keep = 1024, size_t max_capacity = (size_t)8 << 20)
      : max_keep_(max_keep), max_capacity_(max_capacity) {
    free_.reserve(max_keep_);
  }

  // an empty string, with the capacity of a recycled one when there is one
  std::string get() {
    std::lock_guard<std::mutex> lk(mu_);
    if (free_.empty()) {
      ++misses_;
      return std::string();
    }
    std::string s = std::move(free_.back());
    free_.pop_back();
    retained_ -= s.capacity();
    ++hits_;
    return s;
  }

  // return a string's storage (its contents are dropped); called from any thread
  void put(std::string&& s) {
    const size_t cap = s.capacity();
    if (cap <= 64 || cap > max_capacity_) return;  // SSO / outsized: let it go
    s.clear();
    std::lock_guard<std::mutex> lk(mu_);
    if (cap > largest_) largest_ = cap;
    if (free_.size() >= max_keep_) return;  // full: the caller's string keeps (and frees) its storage
    if (slots_ > 0 && retained_ + cap > slots_ * largest_) {  // over the byte budget: freed by the caller
      ++over_budget_;
      return;
    }
    retained_ += cap;
    free_.push_back(std::move(s));
  }

  // byte budget = slots x the largest capacity seen (0: none)
  void set_budget_slots(size_t slots) {
    std::lock_guard<std::mutex> lk(mu_);
    slots_ = slots;
  }
  size_t retained_bytes() const {
    std::lock_guard<std::mutex> lk(mu_);
    return retained_;
  }
  size_t budget_bytes() const {
    std::lock_guard<std::mutex> lk(mu_);
    return slots_ * largest_;
  }
  size_t over_budget() const {
    std::lock_guard<std::mutex> lk(mu_);
    return over_budget_;
  }

  size_t hits() const {
    std::lock_guard<std::mutex> lk(mu_);
    return hits_;
  }
  size_t misses() const {
    std::lock_guard<std::mutex> lk(mu_);
    return misses_;
  }
  size_t kept() const {
    std::lock_guard<std::mutex> lk(mu_);
    return free_.size();
  }

 private:
  mutable std::mutex mu_;
  std::vector<std::string> free_;
  size_t max_keep_, max_capacity_;
  size_t hits_ = 0, misses_ = 0;
  size_t slots_ = 0, largest_ = 0, retained_ = 0, over_budget_ = 0;
};

}  // namespace arena
