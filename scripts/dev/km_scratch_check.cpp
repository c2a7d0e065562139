// Checks the offset arithmetic of KmScratch / KmLists / KmColumns (cryo_ralib_amd/csrc/ralign_scratch.h) on the host, without a device:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Icryo_ralib_amd/csrc \
//         scripts/dev/km_scratch_check.cpp -o km_scratch_check && ./km_scratch_check
//
// For a handful of (n, k, d) it carves the scratch of the five entries that hold member lists the way ralign_embed.hip does,
// backs it with a real allocation of exactly S.off bytes and writes every piece end to end (so the sanitizer sees any piece that
// leaves the allocation), and asserts that every offset is 256-aligned, that no two pieces overlap and that the total is the sum
// of the pieces, each rounded up to 256 bytes.
#include "ralign_scratch.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace ralign;

static const int KM_BLOCK = 1024, VAL_TC = 64, DBS_TC = 64;     // ralign_kmeans.h, ralign_validity.h, ralign_dbscan.h

static int run_len(int n) { const int l = (n + 4095) / 4096; return l > 256 ? l : 256; }    // km_run_len

struct Piece { size_t off, bytes; };

static int failures = 0;

static void check(const char *entry, int n, int k, int d, KmScratch &S, const std::vector<Piece> &pieces)
{
    size_t sum = 0;
    for (const Piece &p : pieces) sum += (p.bytes + 255) / 256 * 256;
    bool ok = sum == S.off;
    std::vector<Piece> sorted = pieces;
    std::sort(sorted.begin(), sorted.end(), [](const Piece &a, const Piece &b) { return a.off < b.off; });
    for (size_t i = 0; i < sorted.size(); ++i) {
        ok = ok && sorted[i].off % 256 == 0 && sorted[i].off + sorted[i].bytes <= S.off;
        if (i + 1 < sorted.size()) ok = ok && sorted[i].off + sorted[i].bytes <= sorted[i + 1].off;
    }
    std::vector<unsigned char> buf(S.off);
    S.base = buf.data();
    for (size_t i = 0; i < pieces.size(); ++i) std::memset(S.at<unsigned char>(pieces[i].off), (int)i + 1, pieces[i].bytes);
    for (size_t i = 0; i < pieces.size(); ++i)              // every piece still holds its own byte: nobody wrote over it
        for (size_t b = 0; b < pieces[i].bytes; b += 97) ok = ok && S.at<unsigned char>(pieces[i].off)[b] == (unsigned char)(i + 1);
    if (!ok) {
        std::printf("FAILED %s n = %d k = %d d = %d: total %zu, pieces %zu\n", entry, n, k, d, S.off, sum);
        ++failures;
    }
}

static std::vector<Piece> lists(const KmLists &M, int n, int k)
{
    const size_t nb = (size_t)(n + KM_BLOCK - 1) / KM_BLOCK;
    std::vector<Piece> p = {{M.o_bcnt, nb * k * 4}, {M.o_cnt, (size_t)k * 4}, {M.o_start, (size_t)k * 4}, {M.o_run0, (size_t)(k + 1) * 4},
                            {M.o_mem, (size_t)n * 4}};
    // the accessors are the offsets
    KmScratch &S = M.S;
    unsigned char *const saved = S.base;
    unsigned char probe;
    S.base = &probe;
    if ((unsigned char *)M.bcnt() != &probe + M.o_bcnt || (unsigned char *)M.cnt() != &probe + M.o_cnt
        || (unsigned char *)M.start() != &probe + M.o_start || (unsigned char *)M.run0() != &probe + M.o_run0
        || (unsigned char *)M.mem() != &probe + M.o_mem) {
        std::printf("FAILED accessors n = %d k = %d\n", n, k);
        ++failures;
    }
    S.base = saved;
    return p;
}

// the pieces of the padded column lists: the member lists, pstart [k + 1] and cols [n + k tc]
static std::vector<Piece> columns(const KmColumns &Cl, int n, int k, int tc)
{
    std::vector<Piece> p = lists(Cl.M, n, k);
    p.push_back({Cl.o_pstart, (size_t)(k + 1) * 4});
    p.push_back({Cl.o_cols, ((size_t)n + (size_t)k * tc) * 4});
    if (Cl.cap != n + k * tc) {
        std::printf("FAILED cap n = %d k = %d\n", n, k);
        ++failures;
    }
    return p;
}

static void one(int n, int k, int d)
{
    const int L = run_len(n), rmax = (n + L - 1) / L + k;
    const bool big = d > 8;                                 // KM_SMALL_D
    {   // ra_kmeans_lloyd (with its own squared norms)
        KmScratch S;
        const KmLists M(S, n, k, KM_BLOCK);
        std::vector<Piece> p = lists(M, n, k);
        for (size_t b : {(size_t)n * 8, (size_t)2 * 4, (size_t)rmax * d * 8, (size_t)k * d * 8, (size_t)k * 8, (size_t)k * 8,
                         big ? (size_t)k * d * 4 : 0, big ? (size_t)k * 4 : 0, big ? (size_t)n * 4 : 0})
            p.push_back({S.take(b), b});
        check("lloyd", n, k, d, S, p);
    }
    {   // ra_kmeans_silhouette
        KmScratch S;
        const KmColumns Cl(S, n, k, KM_BLOCK, VAL_TC);
        check("silhouette", n, k, d, S, columns(Cl, n, k, VAL_TC));
    }
    {   // ra_kmeans_dispersion
        KmScratch S;
        const KmLists M(S, n, k, KM_BLOCK);
        std::vector<Piece> p = lists(M, n, k);
        for (size_t b : {(size_t)rmax * d * 8, (size_t)k * d * 8, (size_t)k * 8, (size_t)n * 8}) p.push_back({S.take(b), b});
        check("dispersion", n, k, d, S, p);
    }
    {   // ra_dbscan_step: the column lists of two "clusters" (core or not), the flags, m and P
        KmScratch S;
        const KmColumns Cl(S, n, 2, KM_BLOCK, DBS_TC);
        std::vector<Piece> p = columns(Cl, n, 2, DBS_TC);
        for (size_t b : {(size_t)n * 4, (size_t)n * 4, (size_t)n * 4}) p.push_back({S.take(b), b});
        check("dbscan_step", n, 2, d, S, p);
    }
    {   // ra_ward_nearest: the column lists of two "clusters" (live or dead) and the flags
        KmScratch S;
        const KmColumns Cl(S, n, 2, KM_BLOCK, DBS_TC);
        std::vector<Piece> p = columns(Cl, n, 2, DBS_TC);
        p.push_back({S.take((size_t)n * 4), (size_t)n * 4});
        check("ward_nearest", n, 2, d, S, p);
    }
}

int main()
{
    const int ns[] = {1, 2, 63, 64, 65, KM_BLOCK - 1, KM_BLOCK, KM_BLOCK + 1, 4 * KM_BLOCK - 1, 4 * KM_BLOCK + 1, 100000};
    const int ks[] = {1, 2, 3, 63, 64, 65, 255, 256};
    const int ds[] = {1, 8, 9, 50};
    int cases = 0;
    for (int n : ns)
        for (int k : ks)
            for (int d : ds) {
                one(n, k, d);
                ++cases;
            }
    std::printf("%d shapes x 5 entries, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
