// staging_layout.hpp -- where the arrays of a one-shot call sit in its one staging block.  No HIP in here: any C++ compiler takes it.
// A block is three consecutive regions: UP (packed on the host, one upload), SCRATCH (the device's own) and DOWN (one download).
// take<T>(n) hands out the byte offset of the next array, on a 16-byte boundary; begin_scratch() and begin_down() close a region
// (a call without scratch goes straight to begin_down()).  ptr<T>(base, offset) is that array in a host or device copy of the block.
#pragma once
#include <cstddef>

namespace qsp {

class StagingLayout {
  public:
    template <typename T>
    size_t take(size_t n) {
        const size_t a = at_;
        at_ = (at_ + n * sizeof(T) + 15) & ~(size_t)15;
        return a;
    }
    void begin_scratch() { up_end_ = at_; in_up_ = false; }
    void begin_down() { if (in_up_) begin_scratch(); down_begin_ = at_; }
    size_t up_bytes() const { return up_end_; }                  // UP is [0, up_bytes())
    size_t down_begin() const { return down_begin_; }            // SCRATCH is [up_bytes(), down_begin())
    size_t down_bytes() const { return at_ - down_begin_; }      // DOWN is [down_begin(), down_begin() + down_bytes())
    size_t in_down(size_t offset) const { return offset - down_begin_; }   // a DOWN array's offset in a host copy of DOWN alone
    size_t total() const { return (at_ + 255) & ~(size_t)255; }  // what to ask the device for

  private:
    size_t at_ = 0, up_end_ = 0, down_begin_ = 0;
    bool in_up_ = true;
};

template <typename T>
T* ptr(void* base, size_t offset) { return reinterpret_cast<T*>(static_cast<char*>(base) + offset); }
template <typename T>
const T* ptr(const void* base, size_t offset) { return reinterpret_cast<const T*>(static_cast<const char*>(base) + offset); }

}  // namespace qsp
