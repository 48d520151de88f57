// Host-side dispatch of the node-wise maps' weight gradients, the message operator's pattern (mpconv_dispatch.h):
// every kernel family of linear_wgrad*.hip has a pure host plan(call, &plan) — 1 = takes the call, 0 = not its shape (FGNN_TRACE
// says why); pointer alignment is checked only when the call carries pointers — and a launch(call, plan): FGNN_OK or < 0.  The
// entry points in linear_wgrad.hip ask the families in one ordered table; no family calls another.  name(call, plan): the kernel
// that launch(call, plan) runs, through the helper the launch itself chooses by (fgnn_linear_wgrad_kernel, include/fgnn_hip_wgrad.h).
#pragma once
#include "fgnn_common.h"

#define WB_MAXSRC 3

// One call: nsrc gradient tensors gy[s] [R][cout[s]] contracted with the same rows x [R][Cin] into gW[s] / gb[s] (gb[s] may be
// NULL).  fgnn_linear_wgrad: nsrc = 1; multi: the merged form of fgnn_linear_wgrad_multi.  x == NULL: a workspace query.
struct FgnnWgradCall {
    const void* x; int64_t R; int Cin, dtype, nsrc; bool multi;
    const void* gy[WB_MAXSRC]; int32_t cout[WB_MAXSRC]; float* gW[WB_MAXSRC]; float* gb[WB_MAXSRC];
    void* workspace; int64_t workspace_bytes; hipStream_t stream;
};

// What a plan chose: the workspace its launch needs, the grid, and the family's few integers.  mode: narrow = x is the narrow
// operand, b16 = the LDS-staged form, general = the vectorised kernel; rows: rows per workgroup (f32, general); aux: b16 = slices
// per workgroup, f32 = input-channel blocks, general = output channels per slice; sb: b16 = the sources' slice ranges.
struct FgnnWgradPlan {
    int64_t ws_bytes; int gx, gy, rows, mode, aux; int sb[WB_MAXSRC + 1];
};

typedef int (*FgnnWgradPlanFn)(const FgnnWgradCall&, FgnnWgradPlan*);
typedef int (*FgnnWgradLaunchFn)(const FgnnWgradCall&, const FgnnWgradPlan&);
typedef const char* (*FgnnWgradNameFn)(const FgnnWgradCall&, const FgnnWgradPlan&);
int fgnn_wgrad_narrow_plan(const FgnnWgradCall& c, FgnnWgradPlan* pl);
int fgnn_wgrad_narrow_launch(const FgnnWgradCall& c, const FgnnWgradPlan& pl);
const char* fgnn_wgrad_narrow_name(const FgnnWgradCall& c, const FgnnWgradPlan& pl);
int fgnn_wgrad_b16_plan(const FgnnWgradCall& c, FgnnWgradPlan* pl);
int fgnn_wgrad_b16_launch(const FgnnWgradCall& c, const FgnnWgradPlan& pl);
const char* fgnn_wgrad_b16_name(const FgnnWgradCall& c, const FgnnWgradPlan& pl);
int fgnn_wgrad_f32_plan(const FgnnWgradCall& c, FgnnWgradPlan* pl);
int fgnn_wgrad_f32_launch(const FgnnWgradCall& c, const FgnnWgradPlan& pl);
const char* fgnn_wgrad_f32_name(const FgnnWgradCall& c, const FgnnWgradPlan& pl);
