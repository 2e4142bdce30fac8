// The host-side rules of a one-shot call (host arrays in, one device block, one upload, the launches, one read-back).
// Plain C++: tests/stage_host_driver.py compiles this file alone, with the address and undefined-behaviour sanitizers.
//
//   layout   the offsets of a call's arrays in its device block: inputs | device-only | outputs | device-only, every array on a
//            256-byte boundary; the inputs go up and the outputs come back as one contiguous range each
//   view     the outputs in the read-back buffer, addressed by their offsets in the block
//   rows     the trial-bound rows of a launch: one row of n + 1 entries per distinct n, shared by the items of that n
//   offsets  what is wrong with an offsets array ptr[0 .. n]
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

namespace xstage {

inline size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// ---- layout
struct Layout {
    size_t off = 0, in_bytes = 0, out0 = 0, out_bytes = 0;
    // an array of `bytes` (an empty one keeps a slot of its own: the kernels get distinct, valid pointers)
    size_t take(size_t bytes) { const size_t o = off; off += align256(bytes > 8 ? bytes : 8); return o; }
    void end_inputs() { in_bytes = off; }                 // what was taken so far is uploaded
    void begin_outputs() { out0 = off; }                  // what is taken from here to end_outputs() is read back
    void end_outputs() { out_bytes = off - out0; }
    size_t total() const { return off; }
};

// ---- view
struct View {
    const unsigned char* back;                            // the read-back buffer: byte 0 is byte out0 of the block
    size_t out0;
    template <typename T> const T* at(size_t offset) const { return reinterpret_cast<const T*>(back + (offset - out0)); }
};

// ---- rows
struct TrialRows {
    std::vector<int32_t> rows;                            // the rows behind one another, in the order of first sight
    std::map<int, int> first;                             // n -> first entry of its row
    // fill_row(n, row) writes row[0 .. n]
    template <typename Fill> int offset_for(int n, Fill&& fill_row) {
        auto it = first.find(n);
        if (it == first.end()) {
            it = first.emplace(n, (int)rows.size()).first;
            rows.resize(rows.size() + (size_t)n + 1);
            fill_row(n, rows.data() + it->second);
        }
        return it->second;
    }
};

// ---- offsets
// null, or what to say after the array's name
template <typename T> inline const char* offsets_fault(const T* ptr, int64_t n) {
    if (ptr[0] != 0) return "does not start at 0";
    for (int64_t j = 0; j < n; ++j)
        if (ptr[j + 1] < ptr[j]) return "decreases";
    return nullptr;
}

}  // namespace xstage
