// library.hip -- what the library says about itself: its C-ABI version and whether the calling thread's device is one it
// was built for.  Host code only, no kernel.
//
// Entry points: mr_abi_version, mr_device_ok.
#include "mr_common.hpp"

extern "C" int mr_abi_version(void) { return MR_ABI_VERSION; }

extern "C" int mr_device_ok(void) {
    // the calling thread's CURRENT device: that is where every entry point of this library launches
    int n = 0, dev = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    const char* a = prop.gcnArchName;
    return (a[0] == 'g' && a[1] == 'f' && a[2] == 'x' && a[3] == '9' && a[4] == '5' && a[5] == '0') ? 1 : 0;
}
