// The slice plan of a block of memory: slices that each start on a 256-byte boundary, in declaration order, and the total - plain
// arithmetic, no context and no HIP include (tests/test_call_block_cpu.py, tests/test_ws_layouts_cpu.py).  For the one-shot calls'
// block (ccal_call.hpp: CallBlock) and for the persistent blocks, which each have ONE layout function ("Persistent blocks").
#pragma once
#include <cassert>
#include <cstddef>
#include <type_traits>

namespace ccal {
template <class T> struct Slice { size_t off = 0, bytes = 0; };        // bytes: rounded up; 0 = absent (an optional slice nobody asked for)

// what a persistent block's slice needs besides room: kCleared - it starts as zeros; kDoubles - doubles the library must write before
// it reads them (the test hook fills them with NaN first; never indices, offsets, counters, flags or DevState)
enum : unsigned { kCleared = 1, kDoubles = 2 };

struct CallPlan {
    struct Range { size_t off = 0, bytes = 0; };
    static constexpr int kMaxPoison = 4;
    size_t total = 0;
    size_t zero_bytes = 0;                 // the cleared slices are declared first: [0, zero_bytes) is ONE clear
    Range poison[kMaxPoison];              // the slices of doubles, neighbours merged
    int n_poison = 0;
    static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
    template <class T, unsigned F = 0> Slice<T> add(size_t count) {
        static_assert(!(F & kDoubles) || std::is_same<T, double>::value, "the poison is a NaN of doubles");
        const Slice<T> s{ total, up256(count * sizeof(T)) };
        total += s.bytes;
        if (F & kCleared) { assert(s.off == zero_bytes && "cleared slices come first"); zero_bytes = total; }
        if ((F & kDoubles) && s.bytes) {
            if (n_poison && poison[n_poison - 1].off + poison[n_poison - 1].bytes == s.off) poison[n_poison - 1].bytes += s.bytes;
            else { assert(n_poison < kMaxPoison); poison[n_poison++] = { s.off, s.bytes }; }
        }
        return s;
    }
};

// a planned block where it lies: the slices' addresses (absent = NULL)
struct Bound { char* base = nullptr; template <class T> T* at(Slice<T> s) const { return s.bytes ? reinterpret_cast<T*>(base + s.off) : nullptr; } };

}  // namespace ccal
