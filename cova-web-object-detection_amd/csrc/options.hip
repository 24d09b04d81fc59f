// Storage of the option state, its one writer cova_set_option (contract: include/cova_hip.h), and the persistent-grid helper that
// reads the grid cap.
#include <stdlib.h>

#include "common.h"
#include "options.h"

CovaOptions g_cova_options;

int cova_internal_persistent_grid(int ntiles, int blocks_per_cu)
{
    // compute units of the CURRENT device (the caller launches under the device guard of its tensors; the host
    // queries run under the same guard): cached per device id, not once per process
    static int cus_of[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    int cus = cus_of[dev];
    if (cus == 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
        if (cus <= 0) cus = 256;
        cus_of[dev] = cus;
    }
    int g = ntiles < cus * blocks_per_cu ? ntiles : cus * blocks_per_cu;
    const int cap = cova_options().grid_cap;
    if (cap > 0 && g > cap) g = cap;
    return g;
}

// Test / A-B hooks, not part of the path's contract.  The state is a per-process constant: mutable until something reads it
// through cova_options(), fixed afterwards -- unless the process opted in with COVA_ALLOW_OPTION_CHANGES=1 (tests, bench.py's
// A/B legs).  Reads the state directly: asking for a change must not itself freeze it.
COVA_API int cova_set_option(int key, int value)
{
    static const struct { int key; int CovaOptions::*field; bool as_bool; } table[] = {
        {2, &CovaOptions::grid_cap, false},      {7, &CovaOptions::conv1_f32, true}, {9, &CovaOptions::wino4_f32, true},
        {14, &CovaOptions::bn1d_variant, false}, {16, &CovaOptions::gat_wide, true}, {22, &CovaOptions::sgemm_dma, true}};
    static const bool allow = [] { const char *e = getenv("COVA_ALLOW_OPTION_CHANGES"); return e != nullptr && e[0] == '1'; }();
    for (const auto &t : table) {
        if (t.key != key) continue;
        if (t.as_bool) value = value != 0;
        if (g_cova_options.*t.field == value) return COVA_OK;
        if (g_cova_options.frozen.load(std::memory_order_relaxed) && !allow) return COVA_ERR_BAD_ARG;
        g_cova_options.*t.field = value;
        return COVA_OK;
    }
    return COVA_ERR_BAD_ARG;
}
