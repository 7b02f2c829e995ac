// The depth of a rendered view, shared by the sources of the map library (through gs2d_map_internal.h) and by the volume
// library (through gs2d_tsdf_rule.h); not part of any C ABI.  Internal linkage: every source compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct DepthCfg { int use_weight_norm; float eps, near, far; };

// The depth of a rendered view (render/__init__.py:129-132): D / (A + eps), zero outside [near, far]; D itself without
// use_weight_norm.  A NaN passes through.
__device__ __forceinline__ float normalised_depth(const DepthCfg& c, float D, float A)
{
    float d = D;
    if (c.use_weight_norm) {
        d = D / (A + c.eps);
        if (d > c.far || d < c.near) d = 0.f;
    }
    return d;
}

}  // namespace
