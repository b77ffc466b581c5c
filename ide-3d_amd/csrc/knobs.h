// knobs.h — EVERY environment switch of libide3d_hip.so, in one table (round 6: the switches used to be 32 scattered getenv calls, some of
// them read per launch).  None of them is needed in production: each selects an arithmetic, a form for devices this library does not tune
// for, or a fallback a test compares against.  The planner's experiment switches (the "before" of rules that were measured and kept) are
// gone; the measurements stay in the rules' comments in modconv.hip.
//
//   read ONCE per process (`knobs()`, first use):
//     IDE3D_CONV_ARITH = fp32 | bf16x6 | bf16x3 | f16x3        process default of ide3d_set_conv_arithmetic (include/ide3d_hip.h)
//     IDE3D_MAPPING_PER_LAYER                                  mapping network as one launch per layer (the form of devices where the one-launch kernel is not co-resident)
//   read PER CALL (`knob_live`): the seven fallbacks that tests/ flip inside one process to compare a lean kernel with the form it replaced
//     IDE3D_FIR_NO_LEAN  IDE3D_FIR_NO_CELL  IDE3D_BIAS_ACT_NO_PLANES  IDE3D_MODCONV_NO_STRIP  IDE3D_MODCONV_PAIR=0|2
//     IDE3D_MODCONV_NO_HEAD_FUSION (ide3d_modconv2d_heads returns IDE3D_ENOKERNEL: the 3x3 layer and its dual heads as two launches)
//     IDE3D_NO_PLANE_GATE (the gated entry points ignore their map: every workgroup of the last backbone block runs, core.hip resolve_plane_gate)
#pragma once
#include <stdlib.h>
#include <string.h>

namespace ide3d {

struct Knobs {
    int conv_arith;                                   // 1 / 3 / 6 / 16
    bool mapping_per_layer;
};

inline const Knobs& knobs() {
    static const Knobs k = [] {
        Knobs k{};
        const char* a = getenv("IDE3D_CONV_ARITH");
        k.conv_arith = !a ? 6 : (!strcmp(a, "fp32") || !strcmp(a, "1")) ? 1 : (!strcmp(a, "bf16x3") || !strcmp(a, "3")) ? 3
                     : (!strcmp(a, "f16x3") || !strcmp(a, "16")) ? 16 : 6;
        k.mapping_per_layer = getenv("IDE3D_MAPPING_PER_LAYER") != nullptr;
        return k;
    }();
    return k;
}

// Not an environment switch but the one measured constant of raster.hip, kept beside the switches so that it is found: a triangle whose
// clipped box holds at least this many samples is rasterized by its whole wave instead of its own lane (ide3d_raster_depth's `large_min`
// argument overrides it; results do not depend on it).  Sweep: scripts/bench_mesh_render.py, DESIGN.md section 5.26.
constexpr int kRasterLargeMin = 256;

// the switches tests flip inside one process: read when asked
inline bool knob_live(const char* name) { return getenv(name) != nullptr; }
inline const char* knob_live_str(const char* name) { return getenv(name); }

}  // namespace ide3d
