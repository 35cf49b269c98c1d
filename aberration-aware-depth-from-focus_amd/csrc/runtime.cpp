// The library's runtime, shared by every unit (no GPU code): the per-thread error string, the ABI version, the device
// query and the events that time the next launch.  See include/aadff.h for the entries.
#include <cstdarg>
#include "common.h"

namespace aadff {

// ------------------------------------------------------------------------------------
// error string shared by the whole library
// ------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// events armed by aadff_time_next_launch for the next stack-convolution / PSF-grid launch of this host thread (common.h)
thread_local hipEvent_t g_time_start = nullptr, g_time_stop = nullptr;

}  // namespace aadff

using namespace aadff;

extern "C" {

int aadff_abi_version(void) { return AADFF_ABI_VERSION; }
const char* aadff_last_error(void) { return g_err; }

int aadff_device_info(int* n_cu, int* lds_bytes, char* arch, int arch_len) {
    int dev = 0;
    AADFF_CHECK_HIP(hipGetDevice(&dev));
    hipDeviceProp_t p;
    AADFF_CHECK_HIP(hipGetDeviceProperties(&p, dev));
    if (n_cu) *n_cu = p.multiProcessorCount;
    if (lds_bytes) *lds_bytes = (int)p.sharedMemPerBlock;
    if (arch && arch_len > 0) {
        std::strncpy(arch, p.gcnArchName, arch_len - 1);
        arch[arch_len - 1] = 0;
    }
    return 0;
}

int aadff_time_next_launch(void* start_event, void* stop_event) {
    AADFF_CHECK_ARG((start_event == nullptr) == (stop_event == nullptr), "time_next_launch: give both events or neither");
    g_time_start = (hipEvent_t)start_event;
    g_time_stop = (hipEvent_t)stop_event;
    return 0;
}

}  // extern "C"
