// Host-side carving of one stream-ordered allocation into aligned pieces (ralign_embed.hip).  Plain C++: no HIP type, so the offset
// arithmetic can be compiled and checked on its own (scripts/dev/km_scratch_check.cpp).
#pragma once
#include <cstddef>

namespace ralign {

// carves aligned pieces out of one stream-ordered allocation
struct KmScratch {
    size_t off = 0;
    unsigned char *base = nullptr;
    size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; }
    template <class T> T *at(size_t o) { return (T *)(base + o); }
};

// the five pieces of the member lists (km_member_lists) of n labels in 0 .. k - 1, histogrammed in blocks of `block` labels:
// bcnt [blocks][k], cnt [k], start [k], run0 [k + 1] and mem [n], all int
struct KmLists {
    KmScratch &S;
    size_t o_bcnt, o_cnt, o_start, o_run0, o_mem;
    KmLists(KmScratch &s, int n, int k, int block)
        : S(s), o_bcnt(s.take((size_t)((n + block - 1) / block) * k * 4)), o_cnt(s.take((size_t)k * 4)), o_start(s.take((size_t)k * 4)),
          o_run0(s.take((size_t)(k + 1) * 4)), o_mem(s.take((size_t)n * 4)) {}
    int *bcnt() const { return S.at<int>(o_bcnt); }
    int *cnt() const { return S.at<int>(o_cnt); }
    int *start() const { return S.at<int>(o_start); }
    int *run0() const { return S.at<int>(o_run0); }
    int *mem() const { return S.at<int>(o_mem); }
};

} // namespace ralign
