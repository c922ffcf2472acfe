// turns.h -- the phase handling shared by the kernels that generate fringe phasors (fringe.hip, psf.hip): a phase in
// TURNS, computed in f64, is reduced to [-1/2, 1/2] and handed to ONE sincos of the working precision.
#pragma once
#include <hip/hip_runtime.h>

namespace rime {

// ---------------------------------------------------------------------------------------
// sin / cos of an angle given in TURNS, |r| <= 1/2: the hardware v_sin_f32 / v_cos_f32 take
// their argument in revolutions; measured max abs error on gfx950 over [-1/2, 1/2] is 1.24e-7
// (profiles/r01_microbench_gfx950.txt) at ~3.2 FMA issue slots each -- versus ~20 slots for a
// quadrant-reduced polynomial of the same accuracy.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void sincos_turns(float r, float& s, float& c)
{
    s = __builtin_amdgcn_sinf(r);
    c = __builtin_amdgcn_cosf(r);
}

__device__ __forceinline__ void sincos_turns(double r, double& s, double& c)
{
    sincospi(2.0 * r, &s, &c);
}

// phase (turns, f64) -> reduced T in [-1/2, 1/2]
template <typename T>
__device__ __forceinline__ T reduce_turns(double ph)
{
    return (T)(ph - rint(ph));
}

} // namespace rime
