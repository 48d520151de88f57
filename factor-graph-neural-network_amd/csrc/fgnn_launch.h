// fgnn_launch.h — the one place where the library launches a kernel, and the one place where a launch failure becomes FGNN_ELAUNCH
// plus a message (host only; included through fgnn_common.h).
#pragma once

static inline hipStream_t fgnn_stream(fgnn_stream_t s) { return static_cast<hipStream_t>(s); }

// hipSuccess -> FGNN_OK (the last error stays as it was); anything else -> "<what> launch: <HIP's text>" and FGNN_ELAUNCH, with the
// thread's sticky HIP error fetched once so that the next library that asks after a launch of its own does not inherit it
static inline int fgnn_launch_status(hipError_t e, const char* what) {
    if (e == hipSuccess) return FGNN_OK;
    fgnn_set_error("%s launch: %s", what, hipGetErrorString(e));
    (void)hipGetLastError();
    return FGNN_ELAUNCH;
}

// a plan-chosen kernel (`fn`) with a caller-built argument array.  Dynamic LDS above 48 KiB is opted into first, every time (no
// per-function cache); at or below 48 KiB no attribute call is made.
static inline int fgnn_launch_fn(const char* what, const void* fn, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, void** args) {
    if (lds_bytes > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) {
            char w[160];
            snprintf(w, sizeof(w), "%s (%zu B LDS)", what, lds_bytes);
            return fgnn_launch_status(e, w);
        }
    }
    return fgnn_launch_status(hipLaunchKernel(fn, grid, block, args, lds_bytes, st), what);
}

template <typename T> struct fgnn_param { typedef T type; };

// a kernel named at the call site: each argument is converted to the kernel's parameter type, as in a <<<>>> launch
template <typename... P>
static inline int fgnn_launch(const char* what, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st,
                              typename fgnn_param<P>::type... p) {
    void* args[] = {(void*)&p..., nullptr};
    return fgnn_launch_fn(what, (const void*)kernel, grid, block, lds_bytes, st, args);
}
