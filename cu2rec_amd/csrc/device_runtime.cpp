// The per-device runtime record of the launch paths (hip_check.hpp: DeviceRuntime) and the fault report that reads it.
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

#include "device.hpp"
#include "hip_check.hpp"

namespace cu2rec {

namespace {
std::mutex g_runtime_mutex;
std::map<int, DeviceRuntime> g_runtime;  // per device (a map: references stay valid while other devices are added)
}  // namespace

std::mutex &device_runtime_mutex() { return g_runtime_mutex; }

DeviceRuntime &device_runtime() {
    int dev = 0;
    CU2REC_HIP(hipGetDevice(&dev));
    DeviceRuntime &r = g_runtime[dev];
    if (r.status) return r;
    unsigned *words = nullptr, *host = nullptr;
    try {
        CU2REC_HIP(hipDeviceGetAttribute(&r.cus, hipDeviceAttributeMultiprocessorCount, dev));
        CU2REC_HIP(hipMalloc(reinterpret_cast<void **>(&words), 128 * sizeof(unsigned)));
        CU2REC_HIP(hipMemset(words, 0, 128 * sizeof(unsigned)));
        CU2REC_HIP(hipHostMalloc(reinterpret_cast<void **>(&host), 2 * sizeof(unsigned), hipHostMallocDefault));
    } catch (...) {  // (nothing kept: the next use tries again)
        if (words) (void)hipFree(words);
        throw;
    }
    host[0] = host[1] = 0;
    r.host_status = host;
    r.probe = words + 64;
    r.status = words;
    return r;
}

namespace {
// the current device's record if it has one (the caller holds g_runtime_mutex); no allocation, no error
DeviceRuntime *existing_device_runtime() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    const auto found = g_runtime.find(dev);
    return found != g_runtime.end() && found->second.status ? &found->second : nullptr;
}
}  // namespace

void check_faults() {
    std::lock_guard<std::mutex> lock(g_runtime_mutex);
    DeviceRuntime *found = existing_device_runtime();
    if (!found) return;
    DeviceRuntime &r = *found;
    volatile unsigned *host = r.host_status;
    if (host[0] != 0) {
        (void)hipDeviceSynchronize();
        (void)hipMemset(r.status + DeviceRuntime::kResidentWord, 0, sizeof(unsigned));
        host[0] = 0;
        fail(CU2REC_EHIP,
             "cu2rec_amd: a persistent SGD launch gave up at its grid barrier (the grid was not co-resident: is another "
             "process or stream using this GPU?); the model state is undefined.  cu2rec_hogwild_resident(0) / "
             "CU2REC_RESIDENT=0 selects the one-launch-per-iteration Hogwild kernel");
    }
    const unsigned bs = host[1];
    if (bs == 0) return;
    (void)hipDeviceSynchronize();
    (void)hipMemset(r.status + DeviceRuntime::kBlocksolveWord, 0, sizeof(unsigned));
    host[1] = 0;
    const char *ordered = "CU2REC_SGD_ORDERED is the same result without concurrent launches";
    if (bs == 2u)  // a look-ahead ring wait (blocksolve_lookahead.hpp, la_wait*): the fork / join had no part in it
        fail(CU2REC_EHIP, std::string("cu2rec_amd: a block-solve iteration gave up at a wait inside a phase-2 workgroup (its wavefronts hand "
                                      "blocks over through flags: is another process or stream holding this GPU's compute units?); the "
                                      "model state is undefined.  ") + ordered);
    // the join gave up.  Self-healing: whatever kept the launches from running side by side will do so again -- every later block-solve
    // call of this process on this device forks and joins with events (unless the environment forces the device form)
    std::string what;
    if (r.topology_forced) {
        what = "(CU2REC_BS_GATE forces the device-side form: unset it to let the library fall back to events.)  ";
    } else if (r.topology == DeviceRuntime::kTopologyEvents) {
        what = "This process already forks and joins the iteration's streams with events.  ";
    } else {
        r.topology = DeviceRuntime::kTopologyEvents;
        r.topology_why = "a device-side join gave up mid-run: switched to the event fork / join";
        what = "From here on this process forks and joins the iteration's streams with events instead of device-side waits (slower by a "
               "few microseconds per iteration, independent of concurrent execution): re-create the model and run again.  ";
    }
    fail(CU2REC_EHIP, "cu2rec_amd: a block-solve iteration gave up waiting for one of its own launches (the three phases of an iteration "
                      "run side by side and hand blocks over through flags: is another process or stream holding this GPU's compute "
                      "units?); the model state is undefined.  " + what + ordered);
}

}  // namespace cu2rec

using namespace cu2rec;

extern "C" {

int cu2rec_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int cu2rec_set_device(int device) {
    return guarded([&] {
        require_device();
        CU2REC_HIP(hipSetDevice(device));
    });
}

int cu2rec_check_faults(void) {
    return guarded([&] {
        require_device();
        CU2REC_HIP(hipDeviceSynchronize());
        check_faults();
    });
}

int cu2rec_blocksolve_topology(char *why, size_t cap) {
    std::string text;
    int mode = -1;
    {
        std::lock_guard<std::mutex> lock(g_runtime_mutex);
        if (const DeviceRuntime *r = existing_device_runtime()) {
            mode = r->topology;
            text = r->topology_why;
        }
    }
    if (why && cap) {
        const size_t n = std::min(text.size(), cap - 1);
        std::memcpy(why, text.data(), n);
        why[n] = 0;
    }
    return mode;
}

}  // extern "C"
