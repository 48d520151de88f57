// Host-side dispatch of the message-passing operator.  Every kernel family of mpconv_fwd*.hip / mpconv_bwd*.hip
// has two functions:
//   plan(call, switches, &plan)  pure host code: 1 = takes the call (plan filled), 0 = not its shape (FGNN_TRACE says why),
//                                < 0 = error.  Pointer alignment is checked only when the call carries pointers.
//   launch(call, plan)           builds the family's parameters from the call and the plan and launches: FGNN_OK or < 0.
// The entry points in mpconv_fwd.hip / mpconv_bwd.hip ask the families in one ordered table; no family calls another.
#pragma once
#include "fgnn_common.h"

struct FgnnFold;

// The environment switches of the dispatch, read once per process (README "Switches").
struct FgnnSwitches {
    bool force_generic;     // FGNN_FORCE_GENERIC
    bool no_ws;             // FGNN_NO_WS
    bool no_bwd_b16;        // FGNN_NO_BWD_B16
    bool no_fwd_hyper;      // FGNN_NO_FWD_HYPER
    bool no_fanin_id;       // FGNN_NO_FANIN_ID
    bool no_ext;            // FGNN_NO_EXT
    bool ext_bf16_split;    // FGNN_EXT_BF16_SPLIT
};
const FgnnSwitches& fgnn_switches();

// One forward call, with every operand an entry point can supply.  stats_epilogue: the BatchNorm statistics of y are asked for
// (stats itself is NULL when fgnn_mpconv_forward_stats_partials plans without pointers); fin / fold_scratch: that BatchNorm is
// finalised inside the launch; add: inference addends of y's layout (fgnn_mpconv_forward_addends).
struct FgnnFwdCall {
    const fgnn_mpconv_desc* d;
    const void* x; const int64_t* idx; const void* et; const float* W; const float* bias;
    const float* pscale; const float* pshift; void* y; uint8_t* argmax;
    bool stats_epilogue; float* stats; const fgnn_bn_final* fin; void* fold_scratch;
    const void* add[3];
    hipStream_t stream;
};

// One backward call; tables: the per-graph tables of fgnn_mpconv_backward_tables (NULL = none).
struct FgnnBwdCall {
    const fgnn_mpconv_desc* d;
    const void* x; const int64_t* idx; const void* et; const float* W; const void* gz; const void* z; const uint8_t* argmax;
    void* gx; void* getype; float* gW; float* gbias; void* workspace; int64_t workspace_bytes;
    const void* tables;
    hipStream_t stream;
};

// What a plan chose: the family (its row in the dispatch table), the kernel, its launch geometry and the few integers its launch
// needs again (their meaning is the family's: kernel mode, split into two launches, edge-type layout, ...).
struct FgnnPlan {
    int family;
    void* fn;
    int grid, block, lds;
    int mode, split, et_mode, aux;
};

typedef int (*FgnnFwdPlanFn)(const FgnnFwdCall&, const FgnnSwitches&, FgnnPlan*);
typedef int (*FgnnFwdLaunchFn)(const FgnnFwdCall&, const FgnnPlan&);
typedef int (*FgnnBwdPlanFn)(const FgnnBwdCall&, const FgnnSwitches&, FgnnPlan*);
typedef int (*FgnnBwdLaunchFn)(const FgnnBwdCall&, const FgnnPlan&);

// ---- forward families (dispatch order: mpconv_fwd.hip) ----
int fgnn_fwd_hyper_plan(const FgnnFwdCall& c, const FgnnSwitches& sw, FgnnPlan* pl);
int fgnn_fwd_hyper_launch(const FgnnFwdCall& c, const FgnnPlan& pl);
int fgnn_fwd_ws_plan(const FgnnFwdCall& c, const FgnnSwitches& sw, FgnnPlan* pl);
int fgnn_fwd_ws_launch(const FgnnFwdCall& c, const FgnnPlan& pl);
int fgnn_fwd_b16_plan(const FgnnFwdCall& c, const FgnnSwitches& sw, FgnnPlan* pl);
int fgnn_fwd_b16_launch(const FgnnFwdCall& c, const FgnnPlan& pl);
int fgnn_fwd_ext_plan(const FgnnFwdCall& c, const FgnnSwitches& sw, FgnnPlan* pl);
int fgnn_fwd_ext_launch(const FgnnFwdCall& c, const FgnnPlan& pl);
int fgnn_fwd_res_plan(const FgnnFwdCall& c, const FgnnSwitches& sw, FgnnPlan* pl);
int fgnn_fwd_res_launch(const FgnnFwdCall& c, const FgnnPlan& pl);

// ---- backward families (dispatch order: mpconv_bwd.hip) ----
int fgnn_bwd_ext_plan(const FgnnBwdCall& c, const FgnnSwitches& sw, FgnnPlan* pl);
int fgnn_bwd_ext_launch(const FgnnBwdCall& c, const FgnnPlan& pl);
int fgnn_bwd_ext_accepts(const fgnn_mpconv_desc* d, const FgnnSwitches& sw);
int fgnn_bwd_hyper_plan(const FgnnBwdCall& c, const FgnnSwitches& sw, FgnnPlan* pl);
int fgnn_bwd_hyper_launch(const FgnnBwdCall& c, const FgnnPlan& pl);
int fgnn_bwd_ws_plan(const FgnnBwdCall& c, const FgnnSwitches& sw, FgnnPlan* pl);
int fgnn_bwd_ws_launch(const FgnnBwdCall& c, const FgnnPlan& pl);
int fgnn_bwd_b16_plan(const FgnnBwdCall& c, const FgnnSwitches& sw, FgnnPlan* pl);
int fgnn_bwd_b16_launch(const FgnnBwdCall& c, const FgnnPlan& pl);
int fgnn_bwd_res_plan(const FgnnBwdCall& c, const FgnnSwitches& sw, FgnnPlan* pl);
int fgnn_bwd_res_launch(const FgnnBwdCall& c, const FgnnPlan& pl);

// ---- shared helpers ----
int fgnn_check_desc(const fgnn_mpconv_desc* d);
void fgnn_stats_upper_half(FgnnFold* fold, fgnn_bn_final* fin);
int64_t fgnn_mpconv_backward_ext_extra_bytes(const fgnn_mpconv_desc* d);
