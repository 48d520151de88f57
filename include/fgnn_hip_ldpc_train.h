/*
 * fgnn_hip_ldpc_train.h — companion of fgnn_hip.h: the two entry points under the LDPC training loop
 * (fgnn_amd/ldpc_train.py; csrc/ldpc_datapath.hip).  Same conventions as the main header: plain pointers, sizes and a hipStream_t;
 * 0 on success, a negative FGNN_E* code otherwise, the message in the thread-local last-error string.  The main header, its list of
 * prototypes and FGNN_ABI_VERSION are unchanged by this file: a library that predates it lacks these two symbols only, and the
 * binding (fgnn_amd/_hip.py: bind_header) reports that as "rebuild" when one of them is called.
 */
#ifndef FGNN_HIP_LDPC_TRAIN_H
#define FGNN_HIP_LDPC_TRAIN_H

#include "fgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * A whole training batch in one launch: `ContinousCodesSP.__getitem__` over B items (/root/reference/lib/data/ldpc_dataset.py:222-236)
 * with the item itself, `gen_data_item` (lib/data/ldpc.py:7-30): a random K-bit message, its codeword [s | G s mod 2] (`s2t`,
 * lib/data/MNC/MNC_py.cpp:22-83), an SNR and a burst level picked from two lists (ldpc_dataset.py:212-221), the channel `t2y`
 * (MNC_py.cpp:86-102) and the model inputs gathered along the incidence lists (ldpc_dataset.py:92-106).
 *
 * Draws.  Per codeword b ONE Philox4x32-10 block, key = seed, counter = (b lo, b hi | 0x80000000, offset lo, offset hi); `offset`
 * is the loop's step number, below 2^63.  The channel's blocks (the same generator, same key) carry the index of a codeword BIT,
 * which is below 2^63, in counter words 0 and 1: the top bit of word 1 keeps this block disjoint from every one of them.
 *     message bit c      bit c of word 0 (c < 32), bit c - 32 of word 1 (32 <= c < 64)
 *     SNR class          snr_choices[(uint64)word 2 * n_snr >> 32]
 *     burst class        sigma_choices[(uint64)word 3 * n_sigma >> 32]
 * The multiply-shift maps 2^32 words onto n classes, so a class holds floor or ceil of 2^32 / n of them: its probability differs
 * from 1 / n by less than 2^-32, i.e. the class index is biased by at most n / 2^32 per class relative to uniform (4e-9 at n = 16).
 * The channel then draws as the rng variant of the channel kernel does for the same (seed, offset): for the codewords and classes
 * drawn here every output equals, bit for bit, what that entry point writes when it is handed them (it IS the same kernel code, with
 * this prologue compiled in).
 *
 * snr_choices [n_snr] and sigma_choices [n_sigma] are HOST arrays of 1..16 values each, copied into the kernel's parameter block.
 * gmask [P] (device): row r of G packed over the K message bits, parity bit r = popcount(gmask[r] & s) & 1.  var_to_factors
 * [K+P][dv], factor_to_vars [nchk][dc] (device, int32).  Outputs: node [B][2][K+P], hop [B][dc][nchk], ef_f2v [B][dc+1][K+P][dv],
 * ef_v2f [B][dc+1][nchk][dc] in `dtype` (FGNN_F32 / FGNN_BF16); snr_db [B], sigma_b [B] f32; and, each where not NULL, cw [B][K+P]
 * uint8 (the codeword), label [B][K] f32 (the message bits, what the loss reads), y [B][K+P] f32 (the received word).
 *
 * K or P outside 1..64, nchk / dv / dc < 1, n_snr or n_sigma above 16, another dtype, B >= 2^31: FGNN_EUNSUPPORTED.  B < 0, n_snr or
 * n_sigma < 1, a null pointer among the required ones: FGNN_EINVAL.  B = 0 is a no-op.  All checks run before any launch.
 */
int fgnn_ldpc_sample_rng(uint64_t seed, uint64_t offset, const float* snr_choices, int32_t n_snr, const float* sigma_choices,
                         int32_t n_sigma, float rho, const uint64_t* gmask, const int32_t* var_to_factors,
                         const int32_t* factor_to_vars, int64_t B, int32_t K, int32_t P, int32_t nchk, int32_t dv, int32_t dc,
                         int32_t dtype, void* node, void* hop, void* ef_f2v, void* ef_v2f, float* snr_db, float* sigma_b,
                         uint8_t* cw, float* label, float* y, fgnn_stream_t stream);

/*
 * The training loss as the script logs it (the loss: /root/reference/train_ldpc.py:222-227; what is logged:
 * train_ldpc.py:232-251): the arguments of the main header's LDPC loss forward, with
 *     out[3]     {total = BCE mean + mse_weight * MSE mean, BCE mean (the script's `loss`), MSE mean (its `sigma_b_loss`)}, f32.
 *                out[0] is bit for bit what the plain loss forward writes: one kernel, the same partials summed in the same order
 *     counts[2]  int64, ADDED to (or NULL): {bits compared, bits where (logit > 0) == (label != 0)} — train_ldpc.py:235-237,
 *                `pred_int = (pred > 0)`: a zero logit of either sign decides 0.  Integer atomics: exact and deterministic.
 * The backward is the plain loss's.  Null pointers, B < 1, n < 1, an unknown dtype, a workspace shorter than the plain loss's
 * workspace size or not 8-byte aligned: FGNN_EINVAL, before any launch.
 */
int fgnn_ldpc_loss_parts_forward(const void* logits, const float* label, const float* pred, const float* sigma_b, int64_t B,
                                 int32_t n, int32_t dtype, float mse_weight, float* out, int64_t* counts, void* workspace,
                                 int64_t workspace_bytes, fgnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
