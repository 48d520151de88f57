// ldpc_word.h — what the LLR-domain kernels (ldpc_llr.hip), the learned min-sum kernels (ldpc_nms.hip, ldpc_nms_layered.hip) and the
// ADMM-LP kernel (ldpc_lp.hip: R holds z, T holds x, prior holds g) share: the limits, the
// per-word LDS layout and the steps every flooding iteration is made of.  Both files are built with -ffp-contract=off and each
// function below keeps its statements in the order the restatements (tests/ldpc_llr_oracle.py, tests/ldpc_nms_oracle.py) pin.
//
// Tables (fgnn_ldpc_decode's): edge e = col_ptr[n] + u is variable n's u-th check; check m's edges are row_edge[row_ptr[m] ..
// row_ptr[m + 1] - 1], their variables row_var[..], in increasing variable order.
//
// Layout: one workgroup works on one word at a time; 64 threads (one wave) for max(N, M) <= 256, 128 for <= 512, 256 above, so a
// lane owns at most four checks and four variables per pass and small codes pay for no barrier between waves.  Per word in LDS,
// in this order: f32 R [E], T [N], prior [N]; the row table packed as edge | var << 16 [E]; the scratch words (4 ints forward: the
// violated checks per wave; 8 floats backward); 16-bit row_ptr [M + 1], col_ptr [N + 1]; then whatever the kernel appends.
#pragma once
#include "fgnn_common.h"
#include <math.h>
#include <stdint.h>

#define LDPC_MAXV 1024      // variables, checks
#define LDPC_MAXD 16        // edges per variable / per check
#define LDPC_CLAMP 4096.0f

extern __shared__ __attribute__((aligned(16))) unsigned char ldpc_lds[];

struct LdpcWord {
    float *R, *T, *prior;       // (the learned backward: gQ, gT, gP)
    uint32_t* rtab; int* wsum;  // wsum: the scratch words
    uint16_t *rp, *cp;
};

// the shape rule: FGNN_OK, or FGNN_EUNSUPPORTED with the message set in ``who``'s name
static int ldpc_word_check_sizes(const char* who, int N, int M, int E) {
    if (N < 1 || N > LDPC_MAXV) FGNN_FAIL(FGNN_EUNSUPPORTED, "%s: N=%d variables outside 1..%d", who, N, LDPC_MAXV);
    if (M < 1 || M > LDPC_MAXV) FGNN_FAIL(FGNN_EUNSUPPORTED, "%s: M=%d checks outside 1..%d", who, M, LDPC_MAXV);
    if (E < 1 || E > (int64_t)LDPC_MAXD * N || E > (int64_t)LDPC_MAXD * M)
        FGNN_FAIL(FGNN_EUNSUPPORTED, "%s: E=%d edges outside 1..%d for N=%d, M=%d (degrees are at most %d)", who, E,
                  LDPC_MAXD * (N < M ? N : M), N, M, LDPC_MAXD);
    return FGNN_OK;
}

static inline int ldpc_word_threads(int N, int M) { const int big = N > M ? N : M; return big <= 256 ? 64 : big <= 512 ? 128 : 256; }

// The two byte counts of the layout (each is what its query has always returned; they round differently).  The LLR kernels': 4
// scratch ints and layer_chk [M], layer_ptr [M + 1] behind col_ptr.  The learned kernels': ``scratch`` bytes, nothing appended.
static inline int64_t ldpc_word_bytes_llr(int N, int M, int E) {
    const int64_t u16s = (int64_t)(M + 1) + (N + 1) + M + (M + 1);
    const int64_t bytes = 4 * (2 * (int64_t)E + 2 * (int64_t)N) + (2 * u16s + 3) / 4 * 4 + 16;
    return (bytes + 15) / 16 * 16;
}
__host__ __device__ static inline int64_t ldpc_word_bytes_nms(int N, int M, int E, int scratch) {
    return (4 * (2 * (int64_t)E + 2 * (int64_t)N) + scratch + 15) / 16 * 16 + (2 * ((int64_t)(M + 1) + (N + 1)) + 15) / 16 * 16;
}

// The ADMM-LP kernel's (ldpc_lp.hip): 16 scratch words, 16-bit row_ptr and col_ptr padded to a whole word, then f32 u [E].
static inline int64_t ldpc_word_bytes_lp(int N, int M, int E) {
    const int64_t bytes = 4 * (2 * (int64_t)E + 2 * (int64_t)N) + 4 * 16 + (2 * ((int64_t)(M + 1) + (N + 1)) + 3) / 4 * 4 + 4 * (int64_t)E;
    return (bytes + 15) / 16 * 16;
}

// ``scratch``: the number of 32-bit scratch words.  What a kernel appends starts at cp + (N + 1).
__device__ __forceinline__ LdpcWord ldpc_word_carve(int N, int M, int E, int scratch) {
    LdpcWord s;
    s.R = (float*)ldpc_lds;
    s.T = s.R + E;
    s.prior = s.T + N;
    s.rtab = (uint32_t*)(s.prior + N);
    s.wsum = (int*)(s.rtab + E);
    s.rp = (uint16_t*)(s.wsum + scratch);
    s.cp = s.rp + (M + 1);
    return s;
}

// the tables into LDS (p: a parameter struct with row_edge, row_var, row_ptr, col_ptr, N, M, E); zero_R: R[e] = 0 on the way
template <class P>
__device__ __forceinline__ void ldpc_stage_tables(const LdpcWord& s, const P& p, bool zero_R) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int e = tid; e < p.E; e += nt) {
        s.rtab[e] = ((uint32_t)p.row_edge[e] & 0xffffu) | ((uint32_t)p.row_var[e] << 16);
        if (zero_R) s.R[e] = 0.0f;
    }
    for (int m = tid; m <= p.M; m += nt) s.rp[m] = (uint16_t)p.row_ptr[m];
    for (int n = tid; n <= p.N; n += nt) s.cp[n] = (uint16_t)p.col_ptr[n];
}

// load: prior[n] = in[n]; NaN -> 0; clamped to +-LDPC_CLAMP.  T[n] = prior[n].
__device__ __forceinline__ void ldpc_load_word(const LdpcWord& s, const float* in, int N) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int n = tid; n < N; n += nt) {
        float v = in[n];
        if (v != v) v = 0.0f;
        v = fminf(fmaxf(v, -LDPC_CLAMP), LDPC_CLAMP);
        s.prior[n] = v;
        s.T[n] = v;
    }
}

// the variable pass for variable n: init + R[col_ptr[n]] + R[col_ptr[n] + 1] + ..., in that order (the forward's total with init =
// prior[n]; the backward's gather of gQ)
__device__ __forceinline__ float ldpc_var_sum(const LdpcWord& s, int n, float init) {
    float sum = init;
    const int e1 = s.cp[n + 1];
    for (int e = s.cp[n]; e < e1; ++e) sum = sum + s.R[e];
    return sum;
}

// viol = the number of checks with an odd number of variables whose hard decision bit(T[var]) is 1: per wave, then over the waves.
// Ends behind a barrier.
template <class Bit>
__device__ __forceinline__ int ldpc_count_violated_by(const LdpcWord& s, int M, Bit bit) {
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    int cnt = 0;
    for (int m0 = wave * 64; m0 < M; m0 += nt) {
        const int m = m0 + lane;
        bool odd = false;
        if (m < M) {
            const int r1 = s.rp[m + 1];
            for (int r = s.rp[m]; r < r1; ++r) odd ^= bit(s.T[s.rtab[r] >> 16]);
        }
        cnt += __popcll(__ballot(odd));
    }
    if (lane == 0) s.wsum[wave] = cnt;
    __syncthreads();                // (the next write of wsum comes after a later barrier: every wave has read it by then)
    int viol = 0;
    for (int w = 0; w < nw; ++w) viol += s.wsum[w];
    return viol;
}

// ... with the LLR-domain decision T[var] < 0
__device__ __forceinline__ int ldpc_count_violated(const LdpcWord& s, int M) {
    return ldpc_count_violated_by(s, M, [](float t) { return t < 0.0f; });
}

// The first sweep of a min-sum check over its edges r0 .. r1 - 1, q = T[var] - R[edge]: the two smallest |q| and their places
// (row-table indices, -1 = none), bit l of signs = (q_l < 0), par = the parity of signs.  A NaN q is skipped by the minima (both
// comparisons are `<`) and counts as non-negative.  What a kernel does not read costs nothing once inlined.
struct LdpcMinScan { float m1, m2; int i1, i2; uint32_t signs; bool par; };

__device__ __forceinline__ LdpcMinScan ldpc_min_scan(const LdpcWord& s, int r0, int r1) {
    float m1 = INFINITY, m2 = INFINITY;
    int i1 = -1, i2 = -1;
    uint32_t signs = 0;
    bool par = false;
    for (int r = r0; r < r1; ++r) {
        const uint32_t ev = s.rtab[r];
        const float q = s.T[ev >> 16] - s.R[ev & 0xffffu];
        const float a = fabsf(q);
        const bool neg = q < 0.0f;
        par ^= neg;
        signs |= (uint32_t)neg << (r - r0);
        if (a < m1) { m2 = m1; i2 = i1; m1 = a; i1 = r; }
        else if (a < m2) { m2 = a; i2 = r; }
    }
    return {m1, m2, i1, i2, signs, par};
}
