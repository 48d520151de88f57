// ldpc_datapath.hip — the LDPC data path in front of the decoder model, on the GPU:
//
//   encode            codeword = [s | G s mod 2]        `s2t(s, 48, 48, Gfile, smn=True)`,
//                                                        /root/reference/lib/data/MNC/MNC_py.cpp:22-83
//   channel           y = 2 gcx (t - 1/2) + z1 (+ gcx sigma_b z2 where u < rho),  gcx = 10^(snr_db/20)
//                                                        `t2y`, MNC_py.cpp:86-102
//   model inputs      node / hop / edge features gathered from y along the code's incidence lists
//                                                        lib/data/ldpc_dataset.py:92-106,222-236
//                     (or from a stored received word: `Codes.__getitem__`, ldpc_dataset.py:141-156)
//
// The reference does this per codeword on the host (a pybind11 call per item, numpy takes, a DataLoader); at
// B = 4096 codewords per step per GPU that is the input bottleneck.  Here a batch is two launches of byte / gather
// work, written once, coalesced, in the storage dtype the model kernels read.  The random draws (z1, u, z2) are
// inputs (the transform is deterministic and is checked bit-for-bit (encode) / to f32 rounding (channel) against
// the oracle) or come from a counter-based generator inside the kernel (fgnn_ldpc_channel_features_rng).  A training loop draws
// the messages and the (SNR, burst) classes in the kernel too: one launch per batch (fgnn_ldpc_sample_rng,
// include/fgnn_hip_ldpc_train.h: ContinousCodesSP.__getitem__ + gen_data_item, lib/data/ldpc.py:7-30, over a batch).
#include "fgnn_common.h"
#include "fgnn_philox.h"
#include "fgnn_hip_ldpc_train.h"
#include "ldpc_features.h"
#include <stdint.h>
#include <type_traits>

// gmask[r] = row r of G packed over the K (<= 64) message bits: parity bit r = popcount(gmask[r] & s) & 1
__global__ __launch_bounds__(LD_THREADS) void ldpc_encode_kernel(const uint8_t* __restrict__ s,
                                                                 const unsigned long long* __restrict__ gmask,
                                                                 int64_t B, int K, int P, uint8_t* __restrict__ cw) {
    __shared__ unsigned long long msg[LD_CW_PER_WG];
    __shared__ unsigned long long gm[64];
    const int64_t b0 = (int64_t)blockIdx.x * LD_CW_PER_WG;
    const int tid = threadIdx.x;
    if (tid < LD_CW_PER_WG) {
        unsigned long long m = 0;
        if (b0 + tid < B) {
            const uint8_t* sp = s + (b0 + tid) * K;
            for (int c = 0; c < K; ++c) m |= (unsigned long long)(sp[c] & 1) << c;
        }
        msg[tid] = m;
    } else if (tid - LD_CW_PER_WG < P) {
        gm[tid - LD_CW_PER_WG] = gmask[tid - LD_CW_PER_WG];
    }
    __syncthreads();
    const int N = K + P;
    const int64_t nb = B - b0 < LD_CW_PER_WG ? B - b0 : LD_CW_PER_WG;
    for (int o = tid; o < nb * N; o += LD_THREADS) {
        const int w = o / N, n = o - w * N;
        const unsigned long long m = msg[w];
        const unsigned bit = n < K ? (unsigned)((m >> n) & 1ull) : (unsigned)(__popcll(m & gm[n - K]) & 1);
        cw[b0 * N + o] = (uint8_t)bit;
    }
}

struct LdFeatParams {
    const uint8_t* cw;           // [B][nvar]
    const float *snr_db, *sigma_b, *z1, *u, *z2;
    const int* var_to_factors;   // [nvar][dv]   (nn_idx_f2v)
    const int* factor_to_vars;   // [nchk][dc]   (nn_idx_v2f)
    float* y;                    // [B][nvar] f32
    void *node, *hop, *ef_f2v, *ef_v2f;
    float rho;
    int nvar, nchk, dv, dc;
    unsigned long long seed, offset;     // RNG variant: Philox key and stream offset (z1 / u / z2 are not read)
};

// What the DRAW prologue of ldpc_features_kernel needs on top (fgnn_ldpc_sample_rng): the code, the class lists (by value, in the
// kernel's parameter block) and where the drawn codewords / classes go.
struct LdDrawParams {
    const unsigned long long* gmask;     // [P]
    float* snr_out;                      // [B]
    float* sb_out;                       // [B]
    uint8_t* cw_out;                     // [B][nvar] or NULL
    float* label_out;                    // [B][K] or NULL
    int K, n_snr, n_sigma;
    float snr_choices[LD_MAX_CHOICES], sigma_choices[LD_MAX_CHOICES];
};
struct LdNoDraw {};

// One workgroup per codeword: y into LDS, then the shared gather stage (ld_gather_features).
// DRAW (fgnn_ldpc_sample_rng; with RNG): cw, snr_db and sigma_b are not read but drawn, from ONE Philox block per codeword —
// counter (b lo, b hi | 0x80000000, offset), disjoint from the channel's blocks below, whose counter words 0, 1 hold a bit index
// < 2^63 — and written out; everything after the prologue is the code the other variants run.
template <typename T, bool RNG, bool DRAW = false>
__global__ __launch_bounds__(LD_THREADS) void ldpc_features_kernel(const LdFeatParams p,
                                                                   const typename std::conditional<DRAW, LdDrawParams, LdNoDraw>::type d) {
    __shared__ float ys[1024];
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, nvar = p.nvar, nchk = p.nchk, dv = p.dv, dc = p.dc;
    float snr = 0.f, sb = 0.f;
    unsigned long long msg = 0;
    if constexpr (DRAW) {
        // nvar = K + P <= 128 here: the threads of the channel loop's one pass each form the codeword's block (10 rounds, no LDS
        // round trip), and ys[nvar] is free to carry the drawn SNR to the gather stage
        if (tid < nvar) {
            unsigned r[4];
            ld_philox((unsigned)b, (unsigned)((unsigned long long)b >> 32) | 0x80000000u, (unsigned)p.offset, (unsigned)(p.offset >> 32),
                      (unsigned)p.seed, (unsigned)(p.seed >> 32), r);
            msg = (unsigned long long)r[0] | ((unsigned long long)r[1] << 32);
            if (d.K < 64) msg &= (1ull << d.K) - 1ull;
            snr = ld_choice(d.snr_choices, (unsigned)(((unsigned long long)r[2] * (unsigned)d.n_snr) >> 32));
            sb = ld_choice(d.sigma_choices, (unsigned)(((unsigned long long)r[3] * (unsigned)d.n_sigma) >> 32));
            if (tid == 0) { d.snr_out[b] = snr; d.sb_out[b] = sb; ys[nvar] = snr; }
        }
    } else {
        snr = p.snr_db[b]; sb = p.sigma_b[b];
    }
    const float gcx = exp2f(snr * 0.16609640474436813f);          // 10^(snr/20) = 2^(snr log2(10)/20)
    for (int n = tid; n < nvar; n += LD_THREADS) {
        const int64_t i = b * nvar + n;
        float z1, u, z2;
        if (RNG) {          // the channel's draws (MNC_py.cpp:89,94-97) from the counter (i, offset): no noise tensors in HBM
            unsigned ra[4], rb[4];
            const unsigned long long ctr = (unsigned long long)i;
            ld_philox((unsigned)ctr, (unsigned)(ctr >> 32), (unsigned)p.offset, (unsigned)(p.offset >> 32), (unsigned)p.seed, (unsigned)(p.seed >> 32), ra);
            ld_philox((unsigned)ctr, (unsigned)(ctr >> 32), (unsigned)p.offset, (unsigned)(p.offset >> 32) ^ 0x80000000u, (unsigned)p.seed, (unsigned)(p.seed >> 32), rb);
            z1 = ld_normal(ra[0], ra[1]);
            u = (float)(ra[2] >> 8) * 5.9604644775390625e-08f;
            z2 = ld_normal(rb[0], rb[1]);
        } else {
            z1 = p.z1[i]; u = p.u[i]; z2 = p.z2[i];
        }
        uint8_t bit;
        if constexpr (DRAW) {           // codeword = [s | G s mod 2] (ldpc_encode_kernel's rule)
            bit = (uint8_t)(n < d.K ? (unsigned)((msg >> n) & 1ull) : (unsigned)(__popcll(msg & d.gmask[n - d.K]) & 1));
            if (d.cw_out) d.cw_out[i] = bit;
            if (d.label_out && n < d.K) d.label_out[b * d.K + n] = (float)bit;
        } else {
            bit = p.cw[i];
        }
        float v = 2.f * gcx * ((float)bit - 0.5f) + z1;
        if (sb >= 1e-20f && u < p.rho) v += gcx * sb * z2;
        ys[n] = v;
        if (!DRAW || p.y) p.y[i] = v;
    }
    __syncthreads();
    ld_gather_features(ys, DRAW ? ys + nvar : p.snr_db + b, 0, p.var_to_factors, p.factor_to_vars, b, nvar, nchk, dv, dc, static_cast<T*>(p.node),
                       static_cast<T*>(p.hop), static_cast<T*>(p.ef_f2v), static_cast<T*>(p.ef_v2f));
}

// Model inputs from a given received word (the reference's `Codes.__getitem__`, lib/data/ldpc_dataset.py:141-156): y into LDS,
// then the same gather as ldpc_features_kernel; node row 1 is snr_db[b * snr_sb + n * snr_sn].
template <typename T>
__global__ __launch_bounds__(LD_THREADS) void ldpc_received_features_kernel(const float* __restrict__ y, const float* __restrict__ snr_db,
                                                                            int64_t snr_sb, int64_t snr_sn, const int* __restrict__ var_to_factors,
                                                                            const int* __restrict__ factor_to_vars, int nvar, int nchk, int dv,
                                                                            int dc, T* node, T* hop, T* ef_f2v, T* ef_v2f) {
    __shared__ float ys[1024];
    const int64_t b = blockIdx.x;
    for (int n = threadIdx.x; n < nvar; n += LD_THREADS) ys[n] = y[b * nvar + n];
    __syncthreads();
    ld_gather_features(ys, snr_db + b * snr_sb, snr_sn, var_to_factors, factor_to_vars, b, nvar, nchk, dv, dc, node, hop, ef_f2v, ef_v2f);
}

// cw [B][K+P] (bytes 0/1) = [s | G s]; s [B][K] bytes, gmask [P] 64-bit rows of G over the K <= 64 message bits.
extern "C" int fgnn_ldpc_encode(const uint8_t* s, const uint64_t* gmask, int64_t B, int K, int P, uint8_t* cw,
                                fgnn_stream_t stream) {
    if (B < 0 || K < 1 || K > 64 || P < 0 || P > 64) FGNN_FAIL(FGNN_EUNSUPPORTED, "ldpc_encode: K=%d P=%d (each <= 64)", K, P);
    if (B == 0) return FGNN_OK;
    if (!s || !gmask || !cw) FGNN_FAIL(FGNN_EINVAL, "ldpc_encode: null pointer");
    const int64_t grid = (B + LD_CW_PER_WG - 1) / LD_CW_PER_WG;
    fgnn_note_kernel("ldpc_encode_kernel");
    return fgnn_launch("ldpc_encode", ldpc_encode_kernel, dim3((unsigned)grid), dim3(LD_THREADS), 0, fgnn_stream(stream), s,
                       (const unsigned long long*)gmask, B, K, P, cw);
}

// Received words and the model's inputs for B codewords of a (nvar, nchk) code with dv checks per variable and dc
// variables per check: y [B][nvar] f32; node [B][2][nvar], hop [B][dc][nchk], ef_f2v [B][dc+1][nvar][dv],
// ef_v2f [B][dc+1][nchk][dc] in `dtype` (FGNN_F32 / FGNN_BF16).
static int ld_channel_launch(bool rng, const uint8_t* cw, const float* snr_db, const float* sigma_b, float rho, const float* z1,
                             const float* u, const float* z2, uint64_t seed, uint64_t offset, const int32_t* var_to_factors,
                             const int32_t* factor_to_vars, int64_t B, int nvar, int nchk, int dv, int dc, int dtype, float* y,
                             void* node, void* hop, void* ef_f2v, void* ef_v2f, fgnn_stream_t stream) {
    if (B < 0 || nvar < 1 || nvar > 1024 || nchk < 1 || dv < 1 || dc < 1 || (dtype != FGNN_F32 && dtype != FGNN_BF16))
        FGNN_FAIL(FGNN_EUNSUPPORTED, "ldpc_channel_features: nvar=%d (<= 1024) nchk=%d dv=%d dc=%d dtype=%d", nvar, nchk, dv,
                  dc, dtype);
    if (B == 0) return FGNN_OK;
    if (!cw || !snr_db || !sigma_b || (!rng && (!z1 || !u || !z2)) || !var_to_factors || !factor_to_vars || !y || !node || !hop ||
        !ef_f2v || !ef_v2f)
        FGNN_FAIL(FGNN_EINVAL, "ldpc_channel_features: null pointer");
    LdFeatParams p = {cw, snr_db, sigma_b, z1, u, z2, var_to_factors, factor_to_vars, y, node, hop, ef_f2v, ef_v2f,
                      rho, nvar, nchk, dv, dc, seed, offset};
    fgnn_note_kernel(rng ? "ldpc_features_kernel<rng>" : "ldpc_features_kernel");
    const dim3 grid((unsigned)B), block(LD_THREADS);
    void (*kernel)(LdFeatParams, LdNoDraw);
    if (dtype == FGNN_F32) kernel = rng ? ldpc_features_kernel<float, true> : ldpc_features_kernel<float, false>;
    else kernel = rng ? ldpc_features_kernel<bf16_t, true> : ldpc_features_kernel<bf16_t, false>;
    return fgnn_launch("ldpc_channel_features", kernel, grid, block, 0, fgnn_stream(stream), p, LdNoDraw{});
}

extern "C" int fgnn_ldpc_channel_features(const uint8_t* cw, const float* snr_db, const float* sigma_b, float rho,
                                          const float* z1, const float* u, const float* z2,
                                          const int32_t* var_to_factors, const int32_t* factor_to_vars, int64_t B,
                                          int nvar, int nchk, int dv, int dc, int dtype, float* y, void* node,
                                          void* hop, void* ef_f2v, void* ef_v2f, fgnn_stream_t stream) {
    return ld_channel_launch(false, cw, snr_db, sigma_b, rho, z1, u, z2, 0, 0, var_to_factors, factor_to_vars, B, nvar, nchk, dv,
                             dc, dtype, y, node, hop, ef_f2v, ef_v2f, stream);
}

// The same with the channel's random draws made in the kernel: Philox4x32-10 keyed by `seed`, counter = (index of the
// codeword bit in the batch, `offset`): z1 = Box-Muller of words 0, 1, u = word 2 / 2^32 (24 bits), z2 = Box-Muller of words
// 0, 1 of the block with the counter's top bit flipped.  A training loop passes its step number as `offset`.
extern "C" int fgnn_ldpc_channel_features_rng(const uint8_t* cw, const float* snr_db, const float* sigma_b, float rho,
                                              uint64_t seed, uint64_t offset, const int32_t* var_to_factors,
                                              const int32_t* factor_to_vars, int64_t B, int nvar, int nchk, int dv, int dc,
                                              int dtype, float* y, void* node, void* hop, void* ef_f2v, void* ef_v2f,
                                              fgnn_stream_t stream) {
    return ld_channel_launch(true, cw, snr_db, sigma_b, rho, nullptr, nullptr, nullptr, seed, offset, var_to_factors,
                             factor_to_vars, B, nvar, nchk, dv, dc, dtype, y, node, hop, ef_f2v, ef_v2f, stream);
}

// A training batch in one launch (include/fgnn_hip_ldpc_train.h): the feature kernel with its DRAW prologue.
extern "C" int fgnn_ldpc_sample_rng(uint64_t seed, uint64_t offset, const float* snr_choices, int n_snr, const float* sigma_choices,
                                    int n_sigma, float rho, const uint64_t* gmask, const int32_t* var_to_factors,
                                    const int32_t* factor_to_vars, int64_t B, int K, int P, int nchk, int dv, int dc, int dtype,
                                    void* node, void* hop, void* ef_f2v, void* ef_v2f, float* snr_db, float* sigma_b, uint8_t* cw,
                                    float* label, float* y, fgnn_stream_t stream) {
    if (B < 0 || n_snr < 1 || n_sigma < 1) FGNN_FAIL(FGNN_EINVAL, "ldpc_sample_rng: B=%lld n_snr=%d n_sigma=%d (B >= 0, lists of >= 1)",
                                                     (long long)B, n_snr, n_sigma);
    if (K < 1 || K > 64 || P < 1 || P > 64 || nchk < 1 || dv < 1 || dc < 1 || n_snr > LD_MAX_CHOICES || n_sigma > LD_MAX_CHOICES ||
        (dtype != FGNN_F32 && dtype != FGNN_BF16) || B > 0x7fffffffll)
        FGNN_FAIL(FGNN_EUNSUPPORTED, "ldpc_sample_rng: K=%d P=%d (each 1..64) nchk=%d dv=%d dc=%d n_snr=%d n_sigma=%d (<= %d) dtype=%d B=%lld",
                  K, P, nchk, dv, dc, n_snr, n_sigma, LD_MAX_CHOICES, dtype, (long long)B);
    if (B == 0) return FGNN_OK;
    if (!snr_choices || !sigma_choices || !gmask || !var_to_factors || !factor_to_vars || !node || !hop || !ef_f2v || !ef_v2f || !snr_db ||
        !sigma_b)
        FGNN_FAIL(FGNN_EINVAL, "ldpc_sample_rng: null pointer");
    const LdFeatParams p = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, var_to_factors, factor_to_vars, y, node, hop, ef_f2v,
                            ef_v2f, rho, K + P, nchk, dv, dc, seed, offset};
    LdDrawParams d = {(const unsigned long long*)gmask, snr_db, sigma_b, cw, label, K, n_snr, n_sigma, {}, {}};
    for (int i = 0; i < n_snr; ++i) d.snr_choices[i] = snr_choices[i];
    for (int i = 0; i < n_sigma; ++i) d.sigma_choices[i] = sigma_choices[i];
    fgnn_note_kernel("ldpc_features_kernel<rng, draw>");
    const dim3 grid((unsigned)B), block(LD_THREADS);
    const auto kernel = dtype == FGNN_F32 ? ldpc_features_kernel<float, true, true> : ldpc_features_kernel<bf16_t, true, true>;
    return fgnn_launch("ldpc_sample_rng", kernel, grid, block, 0, fgnn_stream(stream), p, d);
}

// Model inputs from given received words y [B][nvar] f32 (a stored test set's `noizy_sg`): the outputs of
// fgnn_ldpc_channel_features minus y, node row 1 = snr_db[b * snr_sb + n * snr_sn] (snr_sn = 0: one value per word; snr_sb = nvar,
// snr_sn = 1: the reference's stored per-bit `snr_dbs` rows).
extern "C" int fgnn_ldpc_received_features(const float* y, const float* snr_db, int64_t snr_sb, int64_t snr_sn,
                                           const int32_t* var_to_factors, const int32_t* factor_to_vars, int64_t B, int nvar, int nchk,
                                           int dv, int dc, int dtype, void* node, void* hop, void* ef_f2v, void* ef_v2f,
                                           fgnn_stream_t stream) {
    if (B < 0 || nvar < 1 || nvar > 1024 || nchk < 1 || dv < 1 || dc < 1 || (dtype != FGNN_F32 && dtype != FGNN_BF16))
        FGNN_FAIL(FGNN_EUNSUPPORTED, "ldpc_received_features: nvar=%d (<= 1024) nchk=%d dv=%d dc=%d dtype=%d", nvar, nchk, dv, dc,
                  dtype);
    if (snr_sb < 0 || snr_sn < 0) FGNN_FAIL(FGNN_EINVAL, "ldpc_received_features: negative snr strides");
    if (B == 0) return FGNN_OK;
    if (!y || !snr_db || !var_to_factors || !factor_to_vars || !node || !hop || !ef_f2v || !ef_v2f)
        FGNN_FAIL(FGNN_EINVAL, "ldpc_received_features: null pointer");
    fgnn_note_kernel("ldpc_received_features_kernel");
    const dim3 grid((unsigned)B), block(LD_THREADS);
    hipStream_t st = fgnn_stream(stream);
    if (dtype == FGNN_F32)
        return fgnn_launch("ldpc_received_features", ldpc_received_features_kernel<float>, grid, block, 0, st, y, snr_db, snr_sb, snr_sn, var_to_factors,
                           factor_to_vars, nvar, nchk, dv, dc, (float*)node, (float*)hop, (float*)ef_f2v, (float*)ef_v2f);
    return fgnn_launch("ldpc_received_features", ldpc_received_features_kernel<bf16_t>, grid, block, 0, st, y, snr_db, snr_sb, snr_sn, var_to_factors,
                       factor_to_vars, nvar, nchk, dv, dc, (bf16_t*)node, (bf16_t*)hop, (bf16_t*)ef_f2v, (bf16_t*)ef_v2f);
}

// ---- the training loss behind the decoder (round 5) --------------------------------------------------------------------------------
// /root/reference/train_ldpc.py:222-227:  loss = BCEWithLogits(decoded bits, message bits) + w * MSE(predicted burst amplitude,
// 10^(sigma_b / 20)), both means.  Through torch that is ~12 five-microsecond launches forward and ~13 backward (casts, log-sigmoid,
// two reductions, pow, scalar arithmetic) alone on the GPU between the model's forward and its backward; here two short launches
// forward (per-workgroup sums in double, then the partials in order: a fixed order, bit-reproducible; ONE workgroup for all
// 196 608 logits of the benched size took 193 us, gpurun_out/r05t/timeline) and one backward.
#define LL_THREADS 1024

__device__ __forceinline__ float ll_bce(float x, float y) {       // torch's stable form: max(x,0) - x y + log(1 + exp(-|x|))
    return fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));
}

#define LL_MAXGRID 128

// stage 1: workgroup w sums its grid-stride share of the two terms (double, fixed order) -> part[w][2]
template <typename T>
__global__ __launch_bounds__(LL_THREADS) void ldpc_loss_fwd_kernel(const T* __restrict__ logits, const float* __restrict__ label,
                                                                   const float* __restrict__ pred, const float* __restrict__ sigma_b,
                                                                   int64_t nlogit, int64_t B, double* __restrict__ part,
                                                                   unsigned long long* __restrict__ counts) {
    __shared__ double red[2 * LL_THREADS];
    __shared__ unsigned right_w[LL_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * LL_THREADS;
    double a = 0.0, m = 0.0;
    unsigned right = 0;                 // bits this thread decided as the label says: (logit > 0) == (label != 0), train_ldpc.py:235-237
    for (int64_t i = (int64_t)blockIdx.x * LL_THREADS + tid; i < nlogit; i += step) {
        const float x = fgnn_ld(logits + i), y = label[i];
        a += (double)ll_bce(x, y);
        right += (unsigned)((x > 0.f) == (y != 0.f));
    }
    if (counts) {                       // (uniform) counts[2] += {bits compared, bits right}: a wave's sum by shuffles, the waves' below
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) right += __shfl_xor(right, s);
        if ((tid & 63) == 0) right_w[tid >> 6] = right;
    }
    for (int64_t b = (int64_t)blockIdx.x * LL_THREADS + tid; b < B; b += step) { const float d = pred[b] - powf(10.f, sigma_b[b] * 0.05f); m += (double)(d * d); }
    red[tid] = a; red[LL_THREADS + tid] = m;
    __syncthreads();
    for (int s = LL_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) { red[tid] += red[tid + s]; red[LL_THREADS + tid] += red[LL_THREADS + tid + s]; }
        __syncthreads();
    }
    if (tid == 0) {
        part[2 * blockIdx.x] = red[0]; part[2 * blockIdx.x + 1] = red[LL_THREADS];
        if (counts) {
            unsigned long long r = 0;
            for (int w = 0; w < LL_THREADS / 64; ++w) r += right_w[w];
            if (r) atomicAdd(counts + 1, r);
            if (blockIdx.x == 0) atomicAdd(counts, (unsigned long long)nlogit);
        }
    }
}

// stage 2: the partials in workgroup order; `parts`: loss[1], loss[2] = the two means on their own (fgnn_ldpc_loss_parts_forward)
__global__ __launch_bounds__(64) void ldpc_loss_final_kernel(const double* __restrict__ part, int n, int64_t nlogit, int64_t B, float w,
                                                             float* __restrict__ loss, int parts) {
    if (threadIdx.x != 0) return;
    double a = 0.0, m = 0.0;
    for (int i = 0; i < n; ++i) { a += part[2 * i]; m += part[2 * i + 1]; }
    loss[0] = (float)(a / (double)nlogit + (double)w * m / (double)B);
    if (parts) { loss[1] = (float)(a / (double)nlogit); loss[2] = (float)(m / (double)B); }
}

template <typename T>
__global__ __launch_bounds__(256) void ldpc_loss_bwd_kernel(const T* __restrict__ logits, const float* __restrict__ label,
                                                            const float* __restrict__ pred, const float* __restrict__ sigma_b,
                                                            const float* __restrict__ gloss, int64_t nlogit, int64_t B, float w,
                                                            T* __restrict__ glogits, float* __restrict__ gpred) {
    const float g = gloss[0];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nlogit) {
        const float x = fgnn_ld(logits + i);
        const float sg = 1.f / (1.f + expf(-x));
        fgnn_st(glogits + i, g * (sg - label[i]) / (float)nlogit);
    }
    if (i < B) gpred[i] = g * w * 2.f * (pred[i] - powf(10.f, sigma_b[i] * 0.05f)) / (float)B;
}

static int ll_check(const void* logits, const float* label, const float* pred, const float* sigma_b, int64_t B, int n, int dtype) {
    if (!logits || !label || !pred || !sigma_b) FGNN_FAIL(FGNN_EINVAL, "ldpc_loss: null pointer");
    if (B < 1 || n < 1) FGNN_FAIL(FGNN_EINVAL, "ldpc_loss: bad sizes B=%lld n=%d", (long long)B, n);
    if (dtype != FGNN_F32 && dtype != FGNN_BF16) FGNN_FAIL(FGNN_EINVAL, "ldpc_loss: unknown dtype %d", dtype);
    return FGNN_OK;
}

extern "C" int64_t fgnn_ldpc_loss_workspace_bytes(void) { return (int64_t)LL_MAXGRID * 2 * sizeof(double); }

// Both forward entry points: loss [1] (parts = 0) or [3] (parts = 1), counts [2] or NULL.
static int ll_forward_launch(const void* logits, const float* label, const float* pred, const float* sigma_b, int64_t B, int n, int dtype,
                             float mse_weight, float* loss, int parts, int64_t* counts, void* workspace, int64_t workspace_bytes,
                             fgnn_stream_t stream) {
    int rc = ll_check(logits, label, pred, sigma_b, B, n, dtype);
    if (rc) return rc;
    if (!loss) FGNN_FAIL(FGNN_EINVAL, "ldpc_loss: null pointer");
    if (!workspace || workspace_bytes < fgnn_ldpc_loss_workspace_bytes() || ((uintptr_t)workspace & 7))
        FGNN_FAIL(FGNN_EINVAL, "ldpc_loss: workspace of fgnn_ldpc_loss_workspace_bytes() bytes needed");
    if ((uintptr_t)counts & 7) FGNN_FAIL(FGNN_EINVAL, "ldpc_loss: counts must be 8-byte aligned");
    hipStream_t st = fgnn_stream(stream);
    const int64_t nl = B * n;
    int grid = (int)((nl + 4 * LL_THREADS - 1) / (4 * LL_THREADS));      // ~4 logits per thread (196 608 logits at the benched size: 48 workgroups)
    if (grid > LL_MAXGRID) grid = LL_MAXGRID;
    if (grid < 1) grid = 1;
    double* part = (double*)workspace;
    unsigned long long* cnt = (unsigned long long*)counts;
    rc = dtype == FGNN_F32
        ? fgnn_launch("ldpc_loss forward", ldpc_loss_fwd_kernel<float>, dim3(grid), dim3(LL_THREADS), 0, st, (const float*)logits, label, pred, sigma_b, nl, B, part, cnt)
        : fgnn_launch("ldpc_loss forward", ldpc_loss_fwd_kernel<bf16_t>, dim3(grid), dim3(LL_THREADS), 0, st, (const bf16_t*)logits, label, pred, sigma_b, nl, B, part, cnt);
    if (rc) return rc;
    return fgnn_launch("ldpc_loss forward", ldpc_loss_final_kernel, dim3(1), dim3(64), 0, st, part, grid, nl, B, mse_weight, loss, parts);
}

extern "C" int fgnn_ldpc_loss_forward(const void* logits, const float* label, const float* pred, const float* sigma_b, int64_t B,
                                      int n, int dtype, float mse_weight, float* loss, void* workspace, int64_t workspace_bytes,
                                      fgnn_stream_t stream) {
    return ll_forward_launch(logits, label, pred, sigma_b, B, n, dtype, mse_weight, loss, 0, nullptr, workspace, workspace_bytes, stream);
}

// The loss as the training script logs it (include/fgnn_hip_ldpc_train.h): out[3] = {total, BCE mean, MSE mean}, counts[2] += {bits, bits right}.
extern "C" int fgnn_ldpc_loss_parts_forward(const void* logits, const float* label, const float* pred, const float* sigma_b, int64_t B,
                                            int n, int dtype, float mse_weight, float* out, int64_t* counts, void* workspace,
                                            int64_t workspace_bytes, fgnn_stream_t stream) {
    return ll_forward_launch(logits, label, pred, sigma_b, B, n, dtype, mse_weight, out, 1, counts, workspace, workspace_bytes, stream);
}

extern "C" int fgnn_ldpc_loss_backward(const void* logits, const float* label, const float* pred, const float* sigma_b,
                                       const float* gloss, int64_t B, int n, int dtype, float mse_weight, void* glogits, float* gpred,
                                       fgnn_stream_t stream) {
    int rc = ll_check(logits, label, pred, sigma_b, B, n, dtype);
    if (rc) return rc;
    if (!gloss || !glogits || !gpred) FGNN_FAIL(FGNN_EINVAL, "ldpc_loss: null pointer");
    hipStream_t st = fgnn_stream(stream);
    const int64_t nl = B * n;
    const int grid = (int)((nl + 255) / 256);
    if (dtype == FGNN_F32)
        return fgnn_launch("ldpc_loss backward", ldpc_loss_bwd_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)logits, label, pred, sigma_b, gloss, nl, B, mse_weight, (float*)glogits, gpred);
    return fgnn_launch("ldpc_loss backward", ldpc_loss_bwd_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, (const bf16_t*)logits, label, pred, sigma_b, gloss, nl, B, mse_weight, (bf16_t*)glogits, gpred);
}
