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

// the member lists and, on top of them, the padded column lists (km_column_lists): pstart [k + 1] and cols [cap], every label's
// members in index order in a range padded to a multiple of the column tile tc with -1; cap = n + k tc bounds any padding
struct KmColumns {
    KmLists M;
    int cap;
    size_t o_pstart, o_cols;
    KmColumns(KmScratch &s, int n, int k, int block, int tc)
        : M(s, n, k, block), cap(n + k * tc), o_pstart(s.take((size_t)(k + 1) * 4)), o_cols(s.take((size_t)cap * 4)) {}
    int *pstart() const { return M.S.at<int>(o_pstart); }
    int *cols() const { return M.S.at<int>(o_cols); }
};

} // namespace ralign
