// Stand-alone program of tests/test_launch_helper.py: csrc/fgnn_launch.h on top of csrc/fgnn_api.hip's error plumbing.
// Exit status 0 = every check held; each failed check prints one line.  It decides itself whether a device is present.
#include "fgnn_common.h"
#include <string.h>

__global__ void probe_kernel(int* p, int64_t n) {}

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static bool starts_with(const char* s, const char* head) { return strncmp(s, head, strlen(head)) == 0; }

int main() {
    // ---- the status function on fixed codes: no runtime state involved ----
    fgnn_set_error("sentinel");
    CHECK(fgnn_launch_status(hipSuccess, "probe") == FGNN_OK, "hipSuccess must give FGNN_OK");
    CHECK(strcmp(fgnn_last_error(), "sentinel") == 0, "hipSuccess changed the last error to '%s'", fgnn_last_error());
    const hipError_t codes[] = {hipErrorInvalidValue, hipErrorInvalidConfiguration};
    for (hipError_t code : codes) {
        fgnn_set_error("sentinel");
        CHECK(fgnn_launch_status(code, "probe") == FGNN_ELAUNCH, "HIP error %d must give FGNN_ELAUNCH", (int)code);
        const char* msg = fgnn_last_error();
        CHECK(starts_with(msg, "probe launch: "), "message '%s' does not start with the what string", msg);
        CHECK(strstr(msg, hipGetErrorString(code)) != nullptr, "message '%s' lacks '%s'", msg, hipGetErrorString(code));
        CHECK(strstr(msg, hipGetErrorString(hipSuccess)) == nullptr, "message '%s' carries the text of hipSuccess", msg);
    }

    // ---- the typed launcher on an empty kernel: (nullptr, 3) are converted to (int*, int64_t); 64 KiB takes the LDS opt-in ----
    int ndev = 0;
    const hipError_t dev = hipGetDeviceCount(&ndev);
    const bool have_device = dev == hipSuccess && ndev > 0;
    (void)hipGetLastError();
    const struct { const char* what; size_t lds; } launches[] = {{"probe small", 0}, {"probe large", 64 * 1024}};
    for (const auto& l : launches) {
        fgnn_set_error("sentinel");
        const int rc = fgnn_launch(l.what, probe_kernel, dim3(1), dim3(64), l.lds, fgnn_stream(nullptr), nullptr, 3);
        const char* msg = fgnn_last_error();
        if (have_device) {
            CHECK(rc == FGNN_OK, "%s: rc %d with a device: %s", l.what, rc, msg);
            CHECK(strcmp(msg, "sentinel") == 0, "%s: a launch that succeeded set the message '%s'", l.what, msg);
        } else {
            CHECK(rc == FGNN_ELAUNCH, "%s: rc %d without a device", l.what, rc);
            CHECK(starts_with(msg, l.what), "%s: message '%s' does not start with the what string", l.what, msg);
            CHECK(strstr(msg, " launch: ") != nullptr, "%s: message '%s' lacks ' launch: '", l.what, msg);
            CHECK(strstr(msg, hipGetErrorString(dev == hipSuccess ? hipErrorNoDevice : dev)) != nullptr, "%s: message '%s' lacks HIP's text", l.what, msg);
        }
    }
    if (have_device) CHECK(hipDeviceSynchronize() == hipSuccess, "the empty kernels did not complete");
    printf("%s: %d failure(s)\n", have_device ? "device" : "no device", failures);
    return failures ? 1 : 0;
}
