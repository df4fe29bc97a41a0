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

// The one-shot calls' plan (ccal_call.hpp: CallBlock), which the tests can lay out with guards (CCAL_TEST_GUARD_SLICES in the second
// library); the persistent blocks' plans are plain CallPlans and know nothing of it.  guard_front(gap) in front of the first add() puts
// `gap` bytes at the head of the block, and every present slice is followed by a guard that starts at the slice's EXACT end - the slack
// up to the next 256-byte boundary is part of it - and goes on for `gap` bytes past that boundary.  Slices still start on 256-byte
// boundaries; an absent slice adds nothing.  after: the ordinal of the slice (absent ones count) the guard follows, -1 for the one in
// front.  With gap 0 offsets and total are CallPlan's.
struct GuardedPlan : CallPlan {
    struct Guard { size_t off = 0, bytes = 0; int after = -1; };
    static constexpr int kMaxGuards = 96;  // the largest call has a few dozen slices
    size_t gap = 0;
    Guard guards[kMaxGuards];
    int n_guards = 0, n_slices = 0;
    void guard_front(size_t g) {
        assert(total == 0 && n_slices == 0 && g % 256 == 0 && "in front of the first slice");
        gap = g;
        if (gap) { guards[n_guards++] = { 0, gap, -1 }; total = gap; }
    }
    template <class T> Slice<T> add(size_t count) {      // (a one-shot call's slices carry no flags: poison() and memset() are explicit there)
        const Slice<T> s = CallPlan::add<T>(count);
        const int ordinal = n_slices++;
        if (gap && s.bytes) {
            assert(n_guards < kMaxGuards);
            guards[n_guards++] = { s.off + count * sizeof(T), s.bytes - count * sizeof(T) + gap, ordinal };
            total += gap;
        }
        return s;
    }
};

// a planned block where it lies: the slices' addresses (absent = NULL)
struct Bound { char* base = nullptr; template <class T> T* at(Slice<T> s) const { return s.bytes ? reinterpret_cast<T*>(base + s.off) : nullptr; } };

}  // namespace ccal
