// ldpc_code.hip — the encoder and the one-launch training sampler for ANY regular LDPC code within the data path's limits
// (include/fgnn_hip_ldpc_code.h; fgnn_amd/ldpc_code.py: LdpcCode).  ldpc_datapath.hip's encoder and sampler hold a row of G and a
// message in one 64-bit word (K, P <= 64: the 96.3.963 code the reference is locked to, lib/data/ldpc_dataset.py:11-106) and keep
// their kernels; here both are W = ceil(K / 64) words and a codeword has up to 1024 bits.  The message is kept in LDS by both kernels;
// the rows of G are staged in LDS by the encoder (64 codewords share them) and read from global memory by the sampler (one codeword
// per workgroup reads each row once).  The channel, the gather stage and the generator are the ones of ldpc_datapath.hip
// (ldpc_features.h, fgnn_philox.h).
#include "fgnn_common.h"
#include "fgnn_philox.h"
#include "fgnn_hip_ldpc_code.h"
#include "ldpc_features.h"
#include <stdint.h>

#define LC_MAXVAR 1024
#define LC_MAXW (LC_MAXVAR / 64)

// bit n of the codeword [s | G s mod 2]: m [W] the packed message, g [P][W] the packed rows of G.  The parity of the popcounts over the W
// words is the parity of the popcount of their XOR: one popcount per bit.
__device__ __forceinline__ unsigned lc_bit(const unsigned long long* m, const unsigned long long* g, int n, int K, int W) {
    if (n < K) return (unsigned)((m[n >> 6] >> (n & 63)) & 1ull);
    const unsigned long long* row = g + (int64_t)(n - K) * W;
    unsigned long long acc = 0;
    for (int j = 0; j < W; ++j) acc ^= m[j] & row[j];
    return (unsigned)(__popcll(acc) & 1);
}

// One workgroup per LD_CW_PER_WG codewords, as ldpc_encode_kernel.  Dynamic LDS: msg [64][W] then gm [P][W] 64-bit words, (64 + P) W
// of them: at most 41 400 bytes under K + P <= 1024 (K = 513, P = 511, W = 9), below the 48 KiB a launch gets without asking.
// A message word is one coalesced 64-byte read and a ballot per (codeword, word).
// The workgroup's bytes are one contiguous run that starts 4-byte aligned wherever cw does (64 rows each), whatever the row length: a
// lane forms four consecutive bytes and stores one dword (256 B per wave instruction); wider per lane would have each lane walk 8 or
// 16 rows of G at a stride of W words, which only adds LDS bank conflicts to a kernel that is nowhere near the store rate.
__global__ __launch_bounds__(LD_THREADS) void ldpc_encode_words_kernel(const uint8_t* __restrict__ s,
                                                                       const unsigned long long* __restrict__ gwords, int64_t B, int K,
                                                                       int P, int W, uint8_t* __restrict__ cw) {
    extern __shared__ unsigned long long lc_lds[];
    unsigned long long* msg = lc_lds;
    unsigned long long* gm = lc_lds + LD_CW_PER_WG * W;
    const int64_t b0 = (int64_t)blockIdx.x * LD_CW_PER_WG;
    const int tid = threadIdx.x, lane = tid & 63;
    const int nb = (int)(B - b0 < LD_CW_PER_WG ? B - b0 : LD_CW_PER_WG);
    for (int t = tid >> 6; t < LD_CW_PER_WG * W; t += LD_THREADS / 64) {          // (wave-uniform: every lane takes part in the ballot)
        const int w = t / W, c = 64 * (t - w * W) + lane;
        unsigned bit = 0;
        if (w < nb && c < K) bit = s[(b0 + w) * K + c] & 1u;
        const unsigned long long m = __ballot(bit);
        if (lane == 0) msg[t] = m;
    }
    for (int i = tid; i < P * W; i += LD_THREADS) gm[i] = gwords[i];
    __syncthreads();
    const int N = K + P, total = nb * N;                                            // <= 64 * 1024
    uint8_t* base = cw + b0 * N;
    const int quads = ((uintptr_t)base & 3) == 0 ? total >> 2 : 0;
    for (int q = tid; q < quads; q += LD_THREADS) {
        unsigned v = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int o = 4 * q + i, w = o / N, n = o - w * N;
            v |= lc_bit(msg + w * W, gm, n, K, W) << (8 * i);
        }
        reinterpret_cast<unsigned*>(base)[q] = v;
    }
    for (int o = 4 * quads + tid; o < total; o += LD_THREADS) {
        const int w = o / N, n = o - w * N;
        base[o] = (uint8_t)lc_bit(msg + w * W, gm, n, K, W);
    }
}

struct LcSampleParams {
    const unsigned long long* gwords;    // [P][W]
    const int* var_to_factors;           // [nvar][dv]
    const int* factor_to_vars;           // [nchk][dc]
    float* y;                            // [B][nvar] or NULL
    void *node, *hop, *ef_f2v, *ef_v2f;
    float *snr_out, *sb_out;             // [B]
    uint8_t* cw_out;                     // [B][nvar] or NULL
    float* label_out;                    // [B][K] or NULL
    float rho;
    int K, W, nvar, nchk, dv, dc, n_snr, n_sigma;
    unsigned long long seed, offset;
    float snr_choices[LD_MAX_CHOICES], sigma_choices[LD_MAX_CHOICES];
};

// message word w (bits 64 w .. 64 w + 63 of the message) with the bits at or above K cleared; w < W, so at least one bit stays
__device__ __forceinline__ unsigned long long lc_mask(unsigned long long word, int w, int K) {
    const int keep = K - 64 * w;
    return keep >= 64 ? word : word & ((1ull << keep) - 1ull);
}

// One workgroup per codeword, as ldpc_features_kernel<T, rng, draw>, for nvar up to 1024: the 1 + W / 2 Philox blocks of the codeword
// (include/fgnn_hip_ldpc_code.h) are formed by as many threads and leave the message and the two classes in LDS (words of their own: ys
// holds all 1024 received values at nvar = 1024; the rows of G stay in global memory, this workgroup reads each once), then the channel loop makes as many passes of 256 threads as nvar needs — the
// arithmetic of ldpc_features_kernel's loop, expression for expression, so the bits are its bits — and the shared gather stage follows.
template <typename T>
__global__ __launch_bounds__(LD_THREADS) void ldpc_sample_words_kernel(const LcSampleParams p) {
    __shared__ float ys[LC_MAXVAR];
    __shared__ unsigned long long msg[LC_MAXW];
    __shared__ float cls[2];
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, nvar = p.nvar, K = p.K, W = p.W;
    if (tid < 1 + W / 2) {
        unsigned r[4];
        ld_philox((unsigned)b, 0x80000000u | (unsigned)tid, (unsigned)p.offset, (unsigned)(p.offset >> 32), (unsigned)p.seed,
                  (unsigned)(p.seed >> 32), r);
        const unsigned long long lo = (unsigned long long)r[0] | ((unsigned long long)r[1] << 32);
        if (tid == 0) {
            msg[0] = lc_mask(lo, 0, K);
            const float snr = ld_choice(p.snr_choices, (unsigned)(((unsigned long long)r[2] * (unsigned)p.n_snr) >> 32));
            const float sb = ld_choice(p.sigma_choices, (unsigned)(((unsigned long long)r[3] * (unsigned)p.n_sigma) >> 32));
            cls[0] = snr; cls[1] = sb;
            p.snr_out[b] = snr; p.sb_out[b] = sb;
        } else {
            msg[2 * tid - 1] = lc_mask(lo, 2 * tid - 1, K);
            if (2 * tid < W) msg[2 * tid] = lc_mask((unsigned long long)r[2] | ((unsigned long long)r[3] << 32), 2 * tid, K);
        }
    }
    __syncthreads();
    const float snr = cls[0], sb = cls[1];
    const float gcx = exp2f(snr * 0.16609640474436813f);          // 10^(snr/20) = 2^(snr log2(10)/20)
    for (int n = tid; n < nvar; n += LD_THREADS) {
        const int64_t i = b * nvar + n;
        unsigned ra[4], rb[4];
        const unsigned long long ctr = (unsigned long long)i;
        ld_philox((unsigned)ctr, (unsigned)(ctr >> 32), (unsigned)p.offset, (unsigned)(p.offset >> 32), (unsigned)p.seed, (unsigned)(p.seed >> 32), ra);
        ld_philox((unsigned)ctr, (unsigned)(ctr >> 32), (unsigned)p.offset, (unsigned)(p.offset >> 32) ^ 0x80000000u, (unsigned)p.seed, (unsigned)(p.seed >> 32), rb);
        const float z1 = ld_normal(ra[0], ra[1]);
        const float u = (float)(ra[2] >> 8) * 5.9604644775390625e-08f;
        const float z2 = ld_normal(rb[0], rb[1]);
        const uint8_t bit = (uint8_t)lc_bit(msg, p.gwords, n, K, W);
        if (p.cw_out) p.cw_out[i] = bit;
        if (p.label_out && n < K) p.label_out[b * K + n] = (float)bit;
        float v = 2.f * gcx * ((float)bit - 0.5f) + z1;
        if (sb >= 1e-20f && u < p.rho) v += gcx * sb * z2;
        ys[n] = v;
        if (p.y) p.y[i] = v;
    }
    __syncthreads();
    ld_gather_features(ys, cls, 0, p.var_to_factors, p.factor_to_vars, b, nvar, p.nchk, p.dv, p.dc, static_cast<T*>(p.node),
                       static_cast<T*>(p.hop), static_cast<T*>(p.ef_f2v), static_cast<T*>(p.ef_v2f));
}

extern "C" int fgnn_ldpc_encode_words(const uint8_t* s, const uint64_t* gwords, int64_t B, int K, int P, int W, uint8_t* cw,
                                      fgnn_stream_t stream) {
    if (B < 0) FGNN_FAIL(FGNN_EINVAL, "ldpc_encode_words: B=%lld (>= 0)", (long long)B);
    if (K < 1 || P < 0 || (int64_t)K + P > LC_MAXVAR)
        FGNN_FAIL(FGNN_EUNSUPPORTED, "ldpc_encode_words: K=%d P=%d (K >= 1, P >= 0, K + P <= %d)", K, P, LC_MAXVAR);
    if (W != (K + 63) / 64) FGNN_FAIL(FGNN_EUNSUPPORTED, "ldpc_encode_words: W=%d, K=%d needs W = ceil(K / 64) = %d", W, K, (K + 63) / 64);
    const int64_t grid = (B + LD_CW_PER_WG - 1) / LD_CW_PER_WG;
    if (grid > 0x7fffffffll) FGNN_FAIL(FGNN_EUNSUPPORTED, "ldpc_encode_words: B=%lld (at most 2^31 - 1 workgroups of %d)", (long long)B, LD_CW_PER_WG);
    if (B == 0) return FGNN_OK;
    if (!s || (!gwords && P > 0) || !cw) FGNN_FAIL(FGNN_EINVAL, "ldpc_encode_words: null pointer");
    const size_t lds = (size_t)(LD_CW_PER_WG + P) * W * sizeof(unsigned long long);          // <= 41 400 B (K = 513, P = 511)
    fgnn_note_kernel("ldpc_encode_words_kernel");
    return fgnn_launch("ldpc_encode_words", ldpc_encode_words_kernel, dim3((unsigned)grid), dim3(LD_THREADS), lds, fgnn_stream(stream), s,
                       (const unsigned long long*)gwords, B, K, P, W, cw);
}

extern "C" int fgnn_ldpc_sample_rng_words(uint64_t seed, uint64_t offset, const float* snr_choices, int n_snr, const float* sigma_choices,
                                          int n_sigma, float rho, const uint64_t* gwords, const int32_t* var_to_factors,
                                          const int32_t* factor_to_vars, int64_t B, int K, int P, int W, int nchk, int dv, int dc, int dtype,
                                          void* node, void* hop, void* ef_f2v, void* ef_v2f, float* snr_db, float* sigma_b, uint8_t* cw,
                                          float* label, float* y, fgnn_stream_t stream) {
    if (B < 0 || n_snr < 1 || n_sigma < 1)
        FGNN_FAIL(FGNN_EINVAL, "ldpc_sample_rng_words: B=%lld n_snr=%d n_sigma=%d (B >= 0, lists of >= 1)", (long long)B, n_snr, n_sigma);
    if (K < 1 || P < 1 || (int64_t)K + P > LC_MAXVAR)
        FGNN_FAIL(FGNN_EUNSUPPORTED, "ldpc_sample_rng_words: K=%d P=%d (each >= 1, K + P <= %d)", K, P, LC_MAXVAR);
    if (W != (K + 63) / 64) FGNN_FAIL(FGNN_EUNSUPPORTED, "ldpc_sample_rng_words: W=%d, K=%d needs W = ceil(K / 64) = %d", W, K, (K + 63) / 64);
    if (nchk < 1 || dv < 1 || dc < 1 || n_snr > LD_MAX_CHOICES || n_sigma > LD_MAX_CHOICES || (dtype != FGNN_F32 && dtype != FGNN_BF16) ||
        B > 0x7fffffffll)
        FGNN_FAIL(FGNN_EUNSUPPORTED, "ldpc_sample_rng_words: nchk=%d dv=%d dc=%d n_snr=%d n_sigma=%d (<= %d) dtype=%d B=%lld (< 2^31)", nchk, dv,
                  dc, n_snr, n_sigma, LD_MAX_CHOICES, dtype, (long long)B);
    if (B == 0) return FGNN_OK;
    if (!snr_choices || !sigma_choices || !gwords || !var_to_factors || !factor_to_vars || !node || !hop || !ef_f2v || !ef_v2f || !snr_db ||
        !sigma_b)
        FGNN_FAIL(FGNN_EINVAL, "ldpc_sample_rng_words: null pointer");
    LcSampleParams p = {(const unsigned long long*)gwords, var_to_factors, factor_to_vars, y, node, hop, ef_f2v, ef_v2f, snr_db, sigma_b, cw,
                        label, rho, K, W, K + P, nchk, dv, dc, n_snr, n_sigma, seed, offset, {}, {}};
    for (int i = 0; i < n_snr; ++i) p.snr_choices[i] = snr_choices[i];
    for (int i = 0; i < n_sigma; ++i) p.sigma_choices[i] = sigma_choices[i];
    fgnn_note_kernel("ldpc_sample_words_kernel");
    const dim3 grid((unsigned)B), block(LD_THREADS);
    const auto kernel = dtype == FGNN_F32 ? ldpc_sample_words_kernel<float> : ldpc_sample_words_kernel<bf16_t>;
    return fgnn_launch("ldpc_sample_rng_words", kernel, grid, block, 0, fgnn_stream(stream), p);
}
