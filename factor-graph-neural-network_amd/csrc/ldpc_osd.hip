// ldpc_osd.hip — ordered-statistics reprocessing (Fossorier-Lin OSD of order 0, 1, 2) behind a message-passing LDPC decoder, for a
// batch of words.  The reference has no counterpart; the definition is include/fgnn_hip_ldpc_osd.h's, restated in
// tests/ldpc_osd_oracle.py.  Everything that decides is an integer operation, so the result is defined bit for bit.
//
//   fgnn_ldpc_osd              one launch reprocesses the batch: the best candidate's bits, its cost and its index
//   fgnn_ldpc_osd_lds_bytes    the LDS one word occupies, or < 0 where the shape is not taken
//
// Layout: one workgroup per word, ldpc_word.h's thread rule (64 / 128 / 256), so a thread owns at most OSD_OWN rows and OSD_OWN
// variables, row m belonging to thread m % threads.  Per word in LDS, in this order:
//   mat   u32 [M][RW]   [H | s] bit-packed, column c in bit c & 31 of word c >> 5, s in column N.  RW = ceil((N + 1) / 32) made odd:
//                       the lanes of a wave own consecutive rows, so reading or updating one word of each is bank-conflict free
//   key   u32 [N]       the sort keys w << 10 | n; after the elimination sw[piv_i] per pivot i
//   sw    i32 [N]       the signed weights
//   red   i32 [32]      what crosses waves: C0's parts [0..4), the pivot search's two buffers [8..16), the winner's parts [16..24)
//   ord   u16 [N]       the positions, least reliable first
//   fl    u16 [N]       the non-pivot columns in that order
//   pc    u16 [M]       pivot i's column
//   pr    u16 [M]       pivot i's row; after the elimination bit 15 holds s'_i
//   xb    u8  [N]       h, then x
// At N = M = 1024 that is 152704 bytes of the CU's 160 KiB.
//
// Steps: load and quantise (C0 summed over the workgroup); pass-through words leave here.  Ranks by counting (each thread counts the
// keys below its own: N broadcast reads) give ord.  Each thread builds its rows of [H | s].  Elimination, one barrier per scanned
// column: every thread tests the column's bit in its own rows, a ballot per row slot finds each wave's lowest eligible row, the waves'
// candidates cross in LDS (two buffers, alternating per column, so that the one barrier also separates this column's row updates from
// the last one's) and the lowest row becomes the pivot row; then every thread adds the pivot row to those of its rows that hold the
// bit, word by word.  Once every row is used the remaining columns are non-pivots without a search.  Scoring: one candidate per
// lane walking the pivot rows, then a 64-bit (cost, index) minimum over the workgroup; the winner's flips are applied to xb.
#include "fgnn_hip_ldpc_osd.h"
#include "ldpc_word.h"
#include <limits.h>

#define OSD_OWN 4               // rows / variables a thread owns at most: LDPC_MAXV / 256
#define OSD_MAX_PAIR_SPAN 256   // order 2: at most 256 * 255 / 2 pairs
#define OSD_RED 32

struct OsdParams {
    const float* rel; int64_t rel_sb;
    const float* metric; int64_t metric_sb;
    const int32_t *viol, *row_ptr, *row_var;
    uint8_t* x;
    int32_t *cost, *pattern;
    int N, M, E, order, span;
};

struct OsdLds { uint32_t *mat, *key; int32_t *sw, *red; uint16_t *ord, *fl, *pc, *pr; uint8_t* xb; };

__host__ __device__ static inline int osd_row_words(int N) { return ((N + 32) >> 5) | 1; }

static inline int64_t osd_bytes(int N, int M) {
    const int64_t bytes = 4 * ((int64_t)M * osd_row_words(N) + 2 * (int64_t)N + OSD_RED) + 2 * (2 * (int64_t)N + 2 * (int64_t)M) + N;
    return (bytes + 15) / 16 * 16;
}

__device__ __forceinline__ OsdLds osd_carve(int N, int M, int RW) {
    OsdLds s;
    s.mat = (uint32_t*)ldpc_lds;
    s.key = s.mat + M * RW;
    s.sw = (int32_t*)(s.key + N);
    s.red = s.sw + N;
    s.ord = (uint16_t*)(s.red + OSD_RED);
    s.fl = s.ord + N;
    s.pc = s.fl + N;
    s.pr = s.pc + M;
    s.xb = (uint8_t*)(s.pr + M);
    return s;
}

__device__ __forceinline__ uint32_t osd_q(float v) { return v != v ? 0u : (uint32_t)(fminf(fabsf(v), LDPC_CLAMP) * 256.0f); }

// the cost of the candidate that flips the columns with masks (fw1, fm1), (fw2, fm2) (mask 0: none) besides its pivots, from ``cost``
__device__ __forceinline__ int osd_walk(const OsdLds& s, int RW, int rank, int cost, int fw1, uint32_t fm1, int fw2, uint32_t fm2) {
    for (int i = 0; i < rank; ++i) {
        const uint32_t pr = s.pr[i];
        const uint32_t* row = s.mat + (pr & 0x7fffu) * RW;
        const bool flip = ((pr >> 15) != 0) != ((row[fw1] & fm1) != 0) != ((row[fw2] & fm2) != 0);
        if (flip) cost += (int32_t)s.key[i];
    }
    return cost;
}

__global__ __launch_bounds__(256) void ldpc_osd_kernel(const OsdParams p) {
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const int N = p.N, M = p.M, RW = osd_row_words(N);
    const int64_t b = blockIdx.x;
    const OsdLds s = osd_carve(N, M, RW);

    // load: keys, signed weights, h; C0
    const float* rel = p.rel + b * p.rel_sb;
    const float* met = p.metric ? p.metric + b * p.metric_sb : rel;
    int c0 = 0;
    for (int n = tid; n < N; n += nt) {
        const float r = rel[n], m = met[n];
        const uint32_t w = osd_q(r), wm = osd_q(m);
        const bool h = r < 0.0f, d = h != (m < 0.0f);
        s.key[n] = (w << 10) | (uint32_t)n;
        s.sw[n] = d ? -(int32_t)wm : (int32_t)wm;
        s.xb[n] = h;
        c0 += d ? (int32_t)wm : 0;
    }
    for (int off = 32; off; off >>= 1) c0 += __shfl_xor(c0, off);
    if (lane == 0) s.red[wave] = c0;
    __syncthreads();
    int C0 = 0;
    for (int w = 0; w < nw; ++w) C0 += s.red[w];

    if (p.viol && p.viol[b] == 0) {                 // pass-through (the whole workgroup)
        for (int n = tid; n < N; n += nt) p.x[b * N + n] = s.xb[n];
        if (tid == 0) { p.cost[b] = C0; p.pattern[b] = -1; }
        return;
    }

    // order: rank[n] = the number of keys below key[n] (the keys are distinct)
    {
        uint32_t mine[OSD_OWN];
        int below[OSD_OWN];
#pragma unroll
        for (int k = 0; k < OSD_OWN; ++k) {
            const int n = tid + k * nt;
            mine[k] = n < N ? s.key[n] : 0u;
            below[k] = 0;
        }
        for (int m = 0; m < N; ++m) {
            const uint32_t km = s.key[m];
#pragma unroll
            for (int k = 0; k < OSD_OWN; ++k) below[k] += km < mine[k];
        }
#pragma unroll
        for (int k = 0; k < OSD_OWN; ++k) {
            const int n = tid + k * nt;
            if (n < N) s.ord[below[k]] = (uint16_t)n;
        }
    }
    // [H | s]: each thread its own rows
    for (int m = tid; m < M; m += nt) {
        uint32_t* row = s.mat + m * RW;
        for (int w = 0; w < RW; ++w) row[w] = 0u;
        const int r0 = max(p.row_ptr[m], 0), r1 = min(p.row_ptr[m + 1], p.E);
        uint32_t syn = 0;
        for (int r = r0; r < r1; ++r) {
            const uint32_t v = (uint32_t)p.row_var[r];
            if (v < (uint32_t)N) {
                row[v >> 5] ^= 1u << (v & 31);
                syn ^= s.xb[v];
            }
        }
        row[N >> 5] ^= syn << (N & 31);
    }
    __syncthreads();

    // elimination
    int rank = 0, nf = 0;
    uint32_t used = 0;                              // bit k: my row tid + k * nt is a pivot row
    for (int i = 0; i < N; ++i) {
        const int c = s.ord[i], cw = c >> 5;
        const uint32_t cm = 1u << (c & 31);
        if (rank == M) {                            // every row is used: no pivot can follow
            if (tid == 0) s.fl[nf] = (uint16_t)c;
            ++nf;
            continue;
        }
        uint32_t has = 0;                           // bit k: my row k holds the column
        int cand = INT_MAX;
#pragma unroll
        for (int k = 0; k < OSD_OWN; ++k) {
            const int m = tid + k * nt;
            const bool bit = m < M && (s.mat[m * RW + cw] & cm) != 0;
            has |= (uint32_t)bit << k;
            const unsigned long long el = __ballot(bit && !((used >> k) & 1u));
            if (el && cand == INT_MAX) cand = k * nt + wave * 64 + (__ffsll(el) - 1);
        }
        int* buf = s.red + 8 + (i & 1) * 4;
        if (lane == 0) buf[wave] = cand;
        __syncthreads();
        int pv = INT_MAX;
        for (int w = 0; w < nw; ++w) pv = min(pv, buf[w]);
        if (pv == INT_MAX) {
            if (tid == 0) s.fl[nf] = (uint16_t)c;
            ++nf;
            continue;
        }
        if (tid == 0) { s.pc[rank] = (uint16_t)c; s.pr[rank] = (uint16_t)pv; }
        ++rank;
        const uint32_t* prow = s.mat + pv * RW;
#pragma unroll
        for (int k = 0; k < OSD_OWN; ++k) {
            const int m = tid + k * nt;
            if (m == pv) used |= 1u << k;
            else if ((has >> k) & 1u) {
                uint32_t* row = s.mat + m * RW;
                int w = 0;
                for (; w + 4 <= RW; w += 4) {       // four words in flight: the loop is bound by LDS latency, one wave per SIMD
                    const uint32_t a0 = prow[w], a1 = prow[w + 1], a2 = prow[w + 2], a3 = prow[w + 3];
                    const uint32_t b0 = row[w], b1 = row[w + 1], b2 = row[w + 2], b3 = row[w + 3];
                    row[w] = a0 ^ b0; row[w + 1] = a1 ^ b1; row[w + 2] = a2 ^ b2; row[w + 3] = a3 ^ b3;
                }
                for (; w < RW; ++w) row[w] ^= prow[w];
            }
        }
    }
    __syncthreads();
    // per pivot: its signed weight, and s'_i beside its row
    for (int i = tid; i < rank; i += nt) {
        const uint32_t row = s.pr[i];
        const uint32_t sb = (s.mat[row * RW + (N >> 5)] >> (N & 31)) & 1u;
        s.key[i] = (uint32_t)s.sw[s.pc[i]];
        s.pr[i] = (uint16_t)(row | sb << 15);
    }
    __syncthreads();

    // candidates
    const int L = min(p.span, nf);
    unsigned long long best = ~0ull;
    const int singles = 1 + (p.order >= 1 ? L : 0);
    for (int t = tid; t < singles; t += nt) {
        int cost = C0, fw = 0;
        uint32_t fm = 0;
        if (t) {
            const int f = s.fl[t - 1];
            cost += s.sw[f]; fw = f >> 5; fm = 1u << (f & 31);
        }
        cost = osd_walk(s, RW, rank, cost, fw, fm, 0, 0u);
        const unsigned long long key = (unsigned long long)(uint32_t)cost << 32 | (uint32_t)t;
        best = key < best ? key : best;
    }
    if (p.order == 2) {
        const int pairs = L * (L - 1) / 2;
        int j = 0, o = tid;                         // pair t is (j, j + 1 + o), o < L - 1 - j
        for (int t = tid; t < pairs; t += nt, o += nt) {
            while (o >= L - 1 - j) { o -= L - 1 - j; ++j; }
            const int f1 = s.fl[j], f2 = s.fl[j + 1 + o];
            const int cost = osd_walk(s, RW, rank, C0 + s.sw[f1] + s.sw[f2], f1 >> 5, 1u << (f1 & 31), f2 >> 5, 1u << (f2 & 31));
            const unsigned long long key = (unsigned long long)(uint32_t)cost << 32 | (uint32_t)(1 + L + t);
            best = key < best ? key : best;
        }
    }
    for (int off = 32; off; off >>= 1) {
        const uint32_t hi = (uint32_t)__shfl_xor((int)(best >> 32), off), lo = (uint32_t)__shfl_xor((int)(uint32_t)best, off);
        const unsigned long long other = (unsigned long long)hi << 32 | lo;
        best = other < best ? other : best;
    }
    if (lane == 0) { s.red[16 + 2 * wave] = (int)(best >> 32); s.red[17 + 2 * wave] = (int)(uint32_t)best; }
    __syncthreads();
    best = ~0ull;
    for (int w = 0; w < nw; ++w) {
        const unsigned long long other = (unsigned long long)(uint32_t)s.red[16 + 2 * w] << 32 | (uint32_t)s.red[17 + 2 * w];
        best = other < best ? other : best;
    }

    // the winner's flips
    const int idx = (int)(uint32_t)best;
    int fw1 = 0, fw2 = 0, f1 = -1, f2 = -1;
    uint32_t fm1 = 0, fm2 = 0;
    if (idx >= 1 && idx <= L) f1 = s.fl[idx - 1];
    else if (idx > L) {
        int j = 0, o = idx - 1 - L;
        while (o >= L - 1 - j) { o -= L - 1 - j; ++j; }
        f1 = s.fl[j]; f2 = s.fl[j + 1 + o];
    }
    if (f1 >= 0) { fw1 = f1 >> 5; fm1 = 1u << (f1 & 31); }
    if (f2 >= 0) { fw2 = f2 >> 5; fm2 = 1u << (f2 & 31); }
    for (int i = tid; i < rank; i += nt) {          // (pivot and flipped columns are all different bytes of xb)
        const uint32_t pr = s.pr[i];
        const uint32_t* row = s.mat + (pr & 0x7fffu) * RW;
        if (((pr >> 15) != 0) != ((row[fw1] & fm1) != 0) != ((row[fw2] & fm2) != 0)) s.xb[s.pc[i]] ^= 1;
    }
    if (tid == 0) {
        if (f1 >= 0) s.xb[f1] ^= 1;
        if (f2 >= 0) s.xb[f2] ^= 1;
    }
    __syncthreads();
    for (int n = tid; n < N; n += nt) p.x[b * N + n] = s.xb[n];
    if (tid == 0) { p.cost[b] = (int32_t)(best >> 32); p.pattern[b] = idx; }
}

extern "C" int64_t fgnn_ldpc_osd_lds_bytes(int N, int M) {
    if (N < 1 || N > LDPC_MAXV) { fgnn_set_error("ldpc_osd: N=%d variables outside 1..%d", N, LDPC_MAXV); return -1; }
    if (M < 1 || M > LDPC_MAXV) { fgnn_set_error("ldpc_osd: M=%d checks outside 1..%d", M, LDPC_MAXV); return -1; }
    return osd_bytes(N, M);
}

extern "C" int fgnn_ldpc_osd(const float* rel, int64_t rel_sb, const float* metric, int64_t metric_sb, const int32_t* viol,
                             const int32_t* row_ptr, const int32_t* row_var, int64_t B, int N, int M, int E, int order, int span,
                             uint8_t* x, int32_t* cost, int32_t* pattern, fgnn_stream_t stream) {
    const int rc = ldpc_word_check_sizes("ldpc_osd", N, M, E);
    if (rc != FGNN_OK) return rc;
    if (order < 0 || order > 2) FGNN_FAIL(FGNN_EUNSUPPORTED, "ldpc_osd: order=%d outside 0..2", order);
    if (order == 2 && span > OSD_MAX_PAIR_SPAN)
        FGNN_FAIL(FGNN_EUNSUPPORTED, "ldpc_osd: span=%d above %d with order=2", span, OSD_MAX_PAIR_SPAN);
    if (span < 1) FGNN_FAIL(FGNN_EINVAL, "ldpc_osd: span=%d is below 1", span);
    if (rel_sb < 0 || metric_sb < 0) FGNN_FAIL(FGNN_EINVAL, "ldpc_osd: negative row stride");
    if (B < 0 || B > 0x7fffffffll) FGNN_FAIL(FGNN_EINVAL, "ldpc_osd: batch %lld outside 0 .. 2^31-1", (long long)B);
    if (B == 0) return FGNN_OK;
    if (!rel || !row_ptr || !row_var) FGNN_FAIL(FGNN_EINVAL, "ldpc_osd: null input pointer");
    if (!x || !cost || !pattern) FGNN_FAIL(FGNN_EINVAL, "ldpc_osd: null output pointer");
    OsdParams p = {};
    p.rel = rel; p.rel_sb = rel_sb; p.metric = metric; p.metric_sb = metric_sb; p.viol = viol;
    p.row_ptr = row_ptr; p.row_var = row_var;
    p.x = x; p.cost = cost; p.pattern = pattern;
    p.N = N; p.M = M; p.E = E; p.order = order; p.span = span;
    const int threads = ldpc_word_threads(N, M);
    fgnn_note_kernel("ldpc_osd_kernel<order %d>x%d", order, threads);
    return fgnn_launch("ldpc_osd", ldpc_osd_kernel, dim3((unsigned)B), dim3(threads), (size_t)osd_bytes(N, M), fgnn_stream(stream), p);
}
