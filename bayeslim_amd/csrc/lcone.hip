// lcone.hip -- lightcone sampling of periodic simulation boxes (cosmology.cube2lcone / cube2map; reference cosmology.py:237-427):
// every (radius i, pixel p) output of ONE launch is
//     out[i, p] = sum_{s < S} w[i, s] * sample(sims[cube_idx[i, s]], v_p * dc_i / sim_res)
// with S = 1, 2, 3 cubes per radius (nearest / linear / quadratic radial stencil, table built on the host) and `sample` the
// nearest voxel or the trilinear interpolation of the 8 corners, in a box tiled periodically over all space.  The reference
// builds a whole interpolated cube per radius (b r + c over N^3 voxels) and gathers from it eight times; here no interpolated
// cube and no intermediate of cube size exists: at most 3 x 8 loads per output, nothing else read but the tables.
// A gather: no reduction across lanes, no atomics, no LDS.  Vector ALU only.
//
// Modes.  SPHERE: vec [3][Npix] float64 (the caller's unit vectors), out [Nr][Npix].  PLANE (the reference's angs=None): the
// output pixel (x, y) is the cube's own column, only z = dc / sim_res is sampled, out [Nr][Nx][Ny] (Npix = Nx Ny).
//
// Positions are float64 whatever the cube dtype T: x = (v_x * dc) / sim_res in exactly that order (one product, one quotient,
// nothing to contract), so the voxel of the nearest mode is the reference's bit for bit; at dc / sim_res of a few thousand a
// float32 position would resolve only 5e-4 of a voxel.  Index semantics, per axis of extent N and roll R (0 <= R < N):
//     nearest:  i = rint(x)  (half to even, as np.around)          linear:  i0 = floor(x), f = (T)(x - i0)  (x - i0 is exact
//               in float64 and lies in [0, 1); ONE rounding to T),  i1 = i0 + 1
//     i mod N non-negative (half the sphere has negative coordinates, a shell at dc / sim_res >> N wraps many times), the upper
//     corner (i0 mod N) + 1 wrapped to 0 at N: the reference's ceil whenever f != 0, weight 0 otherwise;
//     the rolled cube at i is the cube at (i - R) mod N: no rolled copy is made.
// |x| is clamped to 9e18 before the conversion to a 64-bit integer (NaN: -9e18): every index is in range for any input.
// Offsets are 64-bit: Nsim Nx Ny Nz exceeds 2^31 at the sizes in use.  z is the contiguous axis; the two z corners of a sample
// are fetched by two loads of one element each (a pair load would be aligned for even z only and would need the wrap path).
//
// Operation order (fixed: the same input gives the same bits from run to run; the error bound of tests/lcone_common.py is
// counted from it).  With g = 1 - f per axis (one rounding each) and lerp(a, b; f, g) = fma(b, f, a * g):
//     c00 = lerp(v000, v100; fx, gx)   c01 = lerp(v001, v101; fx, gx)   c10 = lerp(v010, v110; fx, gx)   c11 = lerp(v011, v111; fx, gx)
//     c0 = lerp(c00, c10; fy, gy)      c1 = lerp(c01, c11; fy, gy)      val = lerp(c0, c1; fz, gz)            (v_xyz, z fastest)
//     acc = (T)w[i, 0] * val_0;   acc = fma((T)w[i, s], val_s, acc)  for s = 1 ... S - 1
// (PLANE: val = lerp(v0, v1; fz, gz) alone.)  With S = 1 the weight is 1 and the nearest mode is a pure gather.
//
// Layout: a lane owns one pixel and a strip of LC_RSTRIP consecutive radii, its unit vector in registers; consecutive lanes
// take consecutive pixels (coalesced stores of every output row), then the next strip: the flat index runs over [strip][pixel].
#include "rime_common.h"

namespace rime {

constexpr int LC_THREADS = 256, LC_RSTRIP = 4, LC_MAXBLOCKS = 1 << 20;

struct LconeArgs {
    const void* sims;                                          // [Nsim][Nx][Ny][Nz] T
    const double* vec;                                         // [3][Npix] (SPHERE)
    const double* dc;                                          // [Nr]
    const int* cube_idx;                                       // [Nr][3]
    const double* weight;                                      // [Nr][3]
    void* out;                                                 // [Nr][Npix] T
    double sim_res;
    int rx, ry, rz, Nsim, Nx, Ny, Nz, Nr, S;
    long long Npix;
};

// i (an integer-valued double, or NaN) modulo N, non-negative
__device__ __forceinline__ int lc_wrap(double i, int N)
{
    const long long m = (long long)fmin(fmax(i, -9.0e18), 9.0e18) % (long long)N;
    return (int)(m < 0 ? m + N : m);
}

// the source index of the rolled cube's index i
__device__ __forceinline__ int lc_src(int i, int roll, int N)
{
    const int s = i - roll;
    return s < 0 ? s + N : s;
}

// the source indices of the one (nearest: s1 unused) or two corners of position x along an axis, and the fraction
template <typename T, bool LINEAR>
__device__ __forceinline__ void lc_axis(double x, int N, int roll, int& s0, int& s1, T& f)
{
    if constexpr (LINEAR) {
        const double fl = floor(x);
        f = (T)(x - fl);
        const int i0 = lc_wrap(fl, N), i1 = i0 + 1 == N ? 0 : i0 + 1;
        s0 = lc_src(i0, roll, N);
        s1 = lc_src(i1, roll, N);
    } else {
        f = (T)0;
        s0 = s1 = lc_src(lc_wrap(rint(x), N), roll, N);
    }
}

template <typename T>
__device__ __forceinline__ T lc_lerp(T a, T b, T f, T g)
{
    return tfma<T>(b, f, a * g);
}

template <typename T, bool PLANE, bool LINEAR>
__global__ __launch_bounds__(LC_THREADS) void lcone_fwd_kernel(LconeArgs A)
{
    const T* sims = reinterpret_cast<const T*>(A.sims);
    T* out = reinterpret_cast<T*>(A.out);
    const size_t Npix = (size_t)A.Npix, nstrip = (size_t)((A.Nr + LC_RSTRIP - 1) / LC_RSTRIP);
    const size_t total = nstrip * Npix, cube = (size_t)A.Nx * A.Ny * A.Nz;
    for (size_t i = (size_t)blockIdx.x * LC_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * LC_THREADS) {
        const size_t pix = i % Npix, strip = i / Npix;
        double vx = 0.0, vy = 0.0, vz = 1.0;
        size_t oxy = 0;                                        // PLANE: the offset of the column (x, y) in a cube
        if constexpr (PLANE) {
            const int px = (int)(pix / (size_t)A.Ny), py = (int)(pix % (size_t)A.Ny);
            oxy = ((size_t)lc_src(px, A.rx, A.Nx) * A.Ny + lc_src(py, A.ry, A.Ny)) * A.Nz;
        } else {
            vx = A.vec[pix]; vy = A.vec[Npix + pix]; vz = A.vec[2 * Npix + pix];
        }
#pragma unroll 1
        for (int k = 0; k < LC_RSTRIP; ++k) {
            const int ir = (int)strip * LC_RSTRIP + k;
            if (ir >= A.Nr) break;
            const double dc = A.dc[ir];
            int z0, z1;
            T fz;
            size_t o00 = oxy, o01 = oxy, o10 = oxy, o11 = oxy;  // offsets of the (x, y) columns: o[x corner][y corner]
            T fx = (T)0, fy = (T)0;
            if constexpr (PLANE) {
                lc_axis<T, LINEAR>(dc / A.sim_res, A.Nz, A.rz, z0, z1, fz);
            } else {
                int x0, x1, y0, y1;
                lc_axis<T, LINEAR>((vx * dc) / A.sim_res, A.Nx, A.rx, x0, x1, fx);
                lc_axis<T, LINEAR>((vy * dc) / A.sim_res, A.Ny, A.ry, y0, y1, fy);
                lc_axis<T, LINEAR>((vz * dc) / A.sim_res, A.Nz, A.rz, z0, z1, fz);
                o00 = ((size_t)x0 * A.Ny + y0) * A.Nz; o01 = ((size_t)x0 * A.Ny + y1) * A.Nz;
                o10 = ((size_t)x1 * A.Ny + y0) * A.Nz; o11 = ((size_t)x1 * A.Ny + y1) * A.Nz;
            }
            const T gx = (T)1 - fx, gy = (T)1 - fy, gz = (T)1 - fz;
            T acc = (T)0;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                if (s < A.S) {
                    const int c = min(max(A.cube_idx[ir * 3 + s], 0), A.Nsim - 1);
                    const T w = (T)A.weight[ir * 3 + s];
                    const T* p = sims + (size_t)c * cube;
                    T val;
                    if constexpr (!LINEAR) {
                        val = p[o00 + z0];
                    } else if constexpr (PLANE) {
                        val = lc_lerp<T>(p[o00 + z0], p[o00 + z1], fz, gz);
                    } else {
                        const T v000 = p[o00 + z0], v001 = p[o00 + z1], v010 = p[o01 + z0], v011 = p[o01 + z1];
                        const T v100 = p[o10 + z0], v101 = p[o10 + z1], v110 = p[o11 + z0], v111 = p[o11 + z1];
                        const T c00 = lc_lerp<T>(v000, v100, fx, gx), c01 = lc_lerp<T>(v001, v101, fx, gx);
                        const T c10 = lc_lerp<T>(v010, v110, fx, gx), c11 = lc_lerp<T>(v011, v111, fx, gx);
                        const T c0 = lc_lerp<T>(c00, c10, fy, gy), c1 = lc_lerp<T>(c01, c11, fy, gy);
                        val = lc_lerp<T>(c0, c1, fz, gz);
                    }
                    acc = s == 0 ? w * val : tfma<T>(w, val, acc);
                }
            }
            out[(size_t)ir * Npix + pix] = acc;
        }
    }
}

} // namespace rime

using namespace rime;

extern "C" int rime_lcone_fwd(int dtype, int mode, int interp, int S, const void* sims, const double* vec, const double* dc,
                              const int* cube_idx, const double* weight, const int* cube_idx_host, double sim_res,
                              int rx, int ry, int rz, int Nsim, int Nx, int Ny, int Nz, int Nr, long long Npix, void* out,
                              void* stream)
{
    if (!real_dtype_ok(dtype)) return RIME_EINVAL;
    if (mode != RIME_LCONE_SPHERE && mode != RIME_LCONE_PLANE) return RIME_EINVAL;
    if (interp != RIME_LCONE_NEAREST && interp != RIME_LCONE_LINEAR) return RIME_EINVAL;
    if (S < 1 || S > 3) return RIME_EINVAL;
    if (Nsim < 1 || Nx < 1 || Ny < 1 || Nz < 1 || Nr < 1 || Npix < 1) return RIME_EINVAL;
    if (!sims || !dc || !cube_idx || !weight || !cube_idx_host || !out) return RIME_EINVAL;
    if (mode == RIME_LCONE_SPHERE && !vec) return RIME_EINVAL;
    if (mode == RIME_LCONE_PLANE && Npix != (long long)Nx * Ny) return RIME_EINVAL;
    if (!(sim_res > 0.0) || !std::isfinite(sim_res)) return RIME_EINVAL;
    if (rx < 0 || rx >= Nx || ry < 0 || ry >= Ny || rz < 0 || rz >= Nz) return RIME_EINVAL;
    const long double lim = 4.0e18L;
    if ((long double)Nsim * Nx * Ny * Nz >= lim || (long double)Nr * Npix >= lim) return RIME_EINVAL;
    for (long long i = 0; i < Nr; ++i)
        for (int s = 0; s < S; ++s)
            if (cube_idx_host[i * 3 + s] < 0 || cube_idx_host[i * 3 + s] >= Nsim) return RIME_EINVAL;
    LconeArgs A{};
    A.sims = sims; A.vec = vec; A.dc = dc; A.cube_idx = cube_idx; A.weight = weight; A.out = out; A.sim_res = sim_res;
    A.rx = rx; A.ry = ry; A.rz = rz; A.Nsim = Nsim; A.Nx = Nx; A.Ny = Ny; A.Nz = Nz; A.Nr = Nr; A.S = S; A.Npix = Npix;
    const long long items = (long long)((Nr + LC_RSTRIP - 1) / LC_RSTRIP) * Npix;
    const int nb = (int)std::min<long long>((items + LC_THREADS - 1) / LC_THREADS, LC_MAXBLOCKS);
    return with_real(dtype, [&](auto t) {
        with_bool(mode == RIME_LCONE_PLANE, [&](auto pl) {
            with_bool(interp == RIME_LCONE_LINEAR, [&](auto li) {
                hipLaunchKernelGGL((lcone_fwd_kernel<decltype(t), decltype(pl)::value, decltype(li)::value>), dim3(nb), dim3(LC_THREADS), 0,
                                   as_stream(stream), A);
            });
        });
        return check_launch();
    });
}
