/*
 * fgnn_hip_ldpc_code.h — companion of fgnn_hip.h: the two entry points that take ANY regular LDPC code within the data path's limits
 * (fgnn_amd/ldpc_code.py: LdpcCode; csrc/ldpc_code.hip).  The main header's encoder and the training header's sampler pack a row of
 * G and a message into ONE 64-bit word (K, P <= 64: MacKay's 96.3.963); here both are W = ceil(K / 64) words (the message in LDS in
 * both kernels; the rows of G in LDS in the encoder, read from global memory in the sampler).  Same conventions as the
 * main header: plain pointers, sizes and a hipStream_t; 0 on success, a negative FGNN_E* code otherwise, the message in the
 * thread-local last-error string.  The main header, its list of prototypes and FGNN_ABI_VERSION are unchanged by this file: a library
 * that predates it lacks these two symbols only, and the binding (fgnn_amd/_hip.py: bind_header) reports that as "rebuild" when one of
 * them is called.  The reference is locked to 96.3.963 (lib/data/ldpc_dataset.py:11-106): these two go beyond it.
 */
#ifndef FGNN_HIP_LDPC_CODE_H
#define FGNN_HIP_LDPC_CODE_H

#include "fgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * cw [B][K+P] (bytes 0/1) = [s | G s mod 2] for messages s [B][K] (bytes; bit = byte & 1).  gwords [P][W] (device): row r of G packed
 * over the K message bits, bit c of the row in bit c % 64 of word c / 64; bits at or above K are zero.  W must be ceil(K / 64).
 * Parity bit r = parity of the popcounts of (gwords[r][j] & message word j) over the W words.  For K, P <= 64 (W = 1) gwords is the
 * main header's gmask and cw equals what its encoder writes, bit for bit.
 *
 * 1 <= K, 0 <= P, K + P <= 1024 (the feature kernels' row), W == ceil(K / 64), at most 2^31 - 1 workgroups of 64 codewords; anything
 * else: FGNN_EUNSUPPORTED with the limit in the message.  B < 0 or a null pointer (gwords may be NULL when P = 0): FGNN_EINVAL.  B = 0
 * is a no-op.  All checks run before the launch.
 */
int fgnn_ldpc_encode_words(const uint8_t* s, const uint64_t* gwords, int64_t B, int32_t K, int32_t P, int32_t W, uint8_t* cw,
                           fgnn_stream_t stream);

/*
 * The one-launch training batch of the training header's sampler for a code of nvar = K + P <= 1024 variables: a random K-bit message
 * per codeword, its codeword [s | G s mod 2], an SNR and a burst class picked from two lists, the channel and the model inputs
 * gathered along the incidence lists.  Arguments and outputs as there, with gwords [P][W] (see above) for gmask and W behind P.
 *
 * Draws.  Philox4x32-10, key = seed.  Block j of codeword b has the counter (b lo, 0x80000000 | j, offset lo, offset hi); `offset` is
 * the loop's step number, below 2^63, and B < 2^31.
 *     block 0      words 0, 1: message word 0 (low 32 bits first);  word 2: SNR class snr_choices[(uint64)word 2 * n_snr >> 32];
 *                  word 3: burst class sigma_choices[(uint64)word 3 * n_sigma >> 32]
 *     block j >= 1 words 0, 1: message word 2j - 1;  words 2, 3: message word 2j  (low 32 bits first; 1 + W / 2 blocks in all)
 * Message bit c is bit c % 64 of message word c / 64; bits at or above K are masked.  Block 0 is the training header's block (B < 2^31:
 * its "b hi" is zero), so for K <= 64 the messages, classes and with them every output are its sampler's, bit for bit.  The channel's
 * blocks (same generator, same key) carry the index of a codeword BIT, below 2^41, in counter words 0 and 1: word 1 is below 2^31
 * there and at or above it here, so the two families of blocks are disjoint.  The channel draws as the rng variant of the channel
 * kernel does for the same (seed, offset): for the codewords and classes drawn here every output equals what that entry point writes
 * when it is handed them.
 *
 * snr_choices [n_snr], sigma_choices [n_sigma]: HOST arrays of 1..16 values.  var_to_factors [K+P][dv], factor_to_vars [nchk][dc]
 * (device, int32).  Outputs: node [B][2][K+P], hop [B][dc][nchk], ef_f2v [B][dc+1][K+P][dv], ef_v2f [B][dc+1][nchk][dc] in `dtype`
 * (FGNN_F32 / FGNN_BF16); snr_db [B], sigma_b [B] f32; and, each where not NULL, cw [B][K+P] uint8, label [B][K] f32 (the message
 * bits), y [B][K+P] f32 (the received word).
 *
 * K < 1, P < 1, K + P > 1024, W != ceil(K / 64), nchk / dv / dc < 1, n_snr or n_sigma above 16, another dtype, B >= 2^31:
 * FGNN_EUNSUPPORTED with the limit in the message.  B < 0, n_snr or n_sigma < 1, a null pointer among the required ones: FGNN_EINVAL.
 * B = 0 is a no-op.  All checks run before the launch.
 */
int fgnn_ldpc_sample_rng_words(uint64_t seed, uint64_t offset, const float* snr_choices, int32_t n_snr, const float* sigma_choices,
                               int32_t n_sigma, float rho, const uint64_t* gwords, const int32_t* var_to_factors,
                               const int32_t* factor_to_vars, int64_t B, int32_t K, int32_t P, int32_t W, int32_t nchk, int32_t dv,
                               int32_t dc, int32_t dtype, void* node, void* hop, void* ef_f2v, void* ef_v2f, float* snr_db,
                               float* sigma_b, uint8_t* cw, float* label, float* y, fgnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
