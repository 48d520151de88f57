/*
 * fgnn_hip_wgrad.h — companion of fgnn_hip.h: which kernel a weight-gradient call of the node-wise maps runs
 * (fgnn_linear_wgrad; csrc/linear_wgrad.hip, linear_wgrad_b16.hip, linear_wgrad_f32.hip).  The main header, its
 * list of prototypes and FGNN_ABI_VERSION are unchanged by this file: a library that predates it lacks this symbol only, and the
 * binding (fgnn_amd/_hip.py: bind_header) reports that as "rebuild" when it is called.
 */
#ifndef FGNN_HIP_WGRAD_H
#define FGNN_HIP_WGRAD_H

#include "fgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The name of the kernel fgnn_linear_wgrad(x, gy, R, Cin, Cout, dtype, ...) would launch, or "" where no family takes the call
 * (fgnn_linear_wgrad then returns FGNN_EUNSUPPORTED) or R, Cin, Cout, dtype are not ones it accepts.  x_low_bits / gy_low_bits: the
 * low four bits of the two data pointers (the plans look at nothing else of them); nothing is dereferenced.  The query walks the
 * same table of families with the same plans as the launch, and each family names its kernel through the helper its launch
 * chooses by, so the two cannot disagree.  Runs on the host like the workspace queries, keeps no state, and does not touch what
 * fgnn_last_kernel reports.  The returned string is static.
 *
 * Names: the kernel's symbol with its template arguments, and for the bf16 family the slices per workgroup its plan chose:
 *
 *     linear_wgrad_kernel<float | bf16>                         general family, scalar loads
 *     linear_wgrad_vec_kernel<float | bf16, 4, 4 | 16, 10>      general family, 16-byte rows
 *     linear_wgrad_b16_narrow_kernel<true | false>              bf16, one operand <= 16 channels (true: x is the narrow one)
 *     linear_wgrad_b16_kernel S=1 | 2 | 4 | 8 | 16              bf16 multiples of 64, register-direct
 *     linear_wgrad_lds_kernel S=8 | 16                          bf16 multiples of 64, LDS-staged
 *     linear_wgrad_f32q_kernel<64 | 128, 64 | 128>              f32 piece form, output block BO x BC
 *
 * No counterpart in the reference (its weight gradients are autograd's): it exists so that a test which means to reach one
 * kernel can assert that it did.
 */
const char* fgnn_linear_wgrad_kernel(int64_t R, int32_t Cin, int32_t Cout, int32_t dtype, int32_t x_low_bits, int32_t gy_low_bits);

#ifdef __cplusplus
}
#endif
#endif
