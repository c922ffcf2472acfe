/*
 * rime_hip.h -- C ABI of the MI355X-native RIME visibility-synthesis library (librime_hip.so)
 *
 * This is the drop-in boundary for the hot path of BayesLIM's `rime_model.RIME.forward`
 * and its autograd backward.  The reference has no FFI: its "interface" for this path is a
 * handful of Python tensor functions.  Each entry point below replaces the arithmetic of the
 * reference function named in its comment (file:line under /root/reference/bayeslim/).
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes; no torch / C++ types.
 *   - every pointer is a DEVICE pointer unless the parameter name ends in `_host`.
 *   - asynchronous on `stream` (a hipStream_t passed as void*); no allocation, no
 *     synchronisation, no host<->device copies: graph-capturable.  Workspace is caller-owned.
 *   - returns 0 on success, a negative RIME_E* code on a rejected call (never throws).
 *   - `dtype`: RIME_F32 (float / complex64) or RIME_F64 (double / complex128) for the
 *     psky / vis / map tensors.  Geometry (blvecs, sdir, freqs) is always float64.
 *   - tensors are dense, last index fastest, layouts given per function.
 */
#ifndef RIME_HIP_H
#define RIME_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RIME_F32 0
#define RIME_F64 1

#define RIME_OK          0
#define RIME_EINVAL     -1   /* bad shape / flag / null pointer            */
#define RIME_EWORKSPACE -2   /* workspace too small                         */
#define RIME_ELAUNCH    -3   /* hipLaunchKernel reported an error           */
#define RIME_EUNSUPPORTED -4

/* library / build identification: "rime_hip <version> gfx950" */
const char* rime_version(void);

/* last HIP error string seen by a failed launch (thread-unsafe diagnostic) */
const char* rime_last_error(void);

/* ---------------------------------------------------------------------------------------
 * Fringe sum, forward.
 *   vis[pp, b, t, f] = sum_p  psky[t, mp(b), pp, f, p] * exp(sign * 2 pi i * freq[f]/c * blvecs[b] . sdir[t, :, p])
 * Replaces: ArrayModel.gen_fringe (telescope_model.py:310-358) fused with the product and
 * pixel sum of RIME._prod_and_sum (rime_model.py:423-429).  The (Nbl, Nf, P) fringe tensor is
 * never materialised.
 *
 *   blvecs   f64 [Nbl, 3]            baseline vectors, ENU metres
 *   sdir     f64 [Nt, 3, Pstride]    unit pointing vectors per time step (x=E, y=N, z=Up);
 *                                    columns p >= npix of a time step must be finite (zero)
 *   freqs    f64 [Nf]                Hz
 *   psky     T   [Nt, Nmp, Npp, Nf, Pstride]      (real)   or
 *            T   [Nt, Nmp, Npp, Nf, Pstride, 2]   (complex, interleaved) perceived sky =
 *                                    apply_beam output per beam-model pair; padded columns 0.
 *            psky_strides_host: NULL for that dense layout, or 4 element strides (HOST)
 *                                    {time, model pair, pol product, channel} of a permuted /
 *                                    strided buffer; the pixel axis is always contiguous.
 *   mp_offsets_host  int[Nmp+1] (HOST) baselines of model pair g are bl_order[off[g] .. off[g+1])
 *   bl_order int [Nbl] or NULL       baseline index per slot (NULL: identity; needs Nmp == 1
 *                                    or baselines already grouped by model pair)
 *   vis      complex<T> [Npp, Nbl, Nt, Nf]  (interleaved re, im)
 *   freq_uniform_host: 0 = arbitrary channel centres (one sincos per element);
 *                    1 = exactly uniform grid freq0_host + k * dfreq_host (rotation recurrence);
 *                    2 = near-uniform: freqs[k] = freq0 + k * dfreq + eps_k with
 *                        2 pi max|eps_k| max_blen / c < 2e-3 (e.g. a float32-rounded linspace):
 *                        recurrence on the fitted grid + first-order per-channel correction.
 *   max_blen_host: upper bound on |blvecs[b]| [m] (<= 0: unknown).  Lets the library pick the
 *                    3-FMA shear rotation when max_blen * |dfreq| / c < 0.3 turn per channel.
 *   workspace: at least rime_fringe_sum_workspace(...) bytes.
 * ------------------------------------------------------------------------------------- */
size_t rime_fringe_sum_workspace(int dtype, int Nbl, int Nt, int Nf, int Pstride,
                                 int Nmp, int Npp, int psky_complex, int backward);

int rime_fringe_sum_fwd(int dtype,
                        const double* blvecs, const double* sdir, const double* freqs,
                        const void* psky, const int* mp_offsets_host, const int* bl_order,
                        int Nbl, int Nt, int Nf, int Pstride, int Nmp, int Npp,
                        int psky_complex, int sign,
                        int freq_uniform_host, double freq0_host, double dfreq_host,
                        double max_blen_host, const long long* psky_strides_host,
                        void* vis, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fringe sum, backward (gradient w.r.t. psky; PyTorch convention grad = dL/dRe + i dL/dIm):
 *   gpsky[t, mp, pp, f, p] = sum_{b in group mp} conj(F[b,t,f,p]) * gvis[pp, b, t, f]
 *   (real part only when psky is real).  Regenerates the fringe; deterministic (no atomics).
 * Replaces the autograd backward of rime_model.py:429 (SumBackward/MulBackward over the
 * saved (Nbl,Nf,P) fringe and psky tensors).
 *   gvis  complex<T> [Npp, Nbl, Nt, Nf];  gpsky same layout as psky (fully overwritten).
 * ------------------------------------------------------------------------------------- */
int rime_fringe_sum_bwd(int dtype,
                        const double* blvecs, const double* sdir, const double* freqs,
                        const void* gvis, const int* mp_offsets_host, const int* bl_order,
                        int Nbl, int Nt, int Nf, int Pstride, int Nmp, int Npp,
                        int psky_complex, int sign,
                        int freq_uniform_host, double freq0_host, double dfreq_host,
                        double max_blen_host, const long long* gpsky_strides_host,
                        void* gpsky, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Antenna-factored fringe sum on the matrix cores (float32, one beam-model pair).  Same result as rime_fringe_sum_fwd/bwd for baselines that are antenna
 * pairs: with E_a = exp(sign 2 pi i nu r_a.s / c) the fringe of baseline (a1 -> a2) is
 * E_a2 conj(E_a1), so per (time, channel) all visibilities are one Hermitian rank-P update
 * V = E^H diag(psky) E, computed on v_mfma_f32_32x32x16_f16 with an f16 hi/lo split of the f32
 * operands (three cross products, f32 accumulation).  Replaces the same reference lines as
 * rime_fringe_sum_fwd/bwd.
 *   antpos f64 [Nant, 3] ENU metres; psky / gpsky f32 [t][f][p] with element strides st_t, st_f,
 *       st_p (1, or 2 for the real / imaginary plane of an interleaved complex buffer).  One call
 *       handles one real plane: polarisation products and the two planes of a complex psky are
 *       separate calls (V is linear in psky: V[ar + i ai] = V[ar] + i V[ai])
 *   scale / gscale f32 [Nt, Nf]: power-of-two factors that bring max|psky[t,f,:]| (resp.
 *       max|gvis[:,t,f]|) to ~2^14 -- computed by the caller (a torch amax), exact to undo
 *   rowmin f32 [Nt, Nf] or NULL (forward): min of each psky row; rows with min >= 0 run without the
 *       per-pixel sign masks (NULL: every row is treated as signed)
 *   pair_direct / pair_conj int32 [128*128]: for antenna indices (i, j) with tile(i) <= tile(j)
 *       (tile = index / 32) the baseline slot that receives V[i,j] (pair stored as i -> j) and the
 *       slot that receives conj(V[i,j]) (pair stored as j -> i, only when tile(j) > tile(i)), or -1
 *   vis / gvis complex64 [Nbl, Nt, Nf]
 * ------------------------------------------------------------------------------------- */
size_t rime_fringe_ant_workspace(int Nbl, int Nt, int Nf, int Pstride);   /* forward: per-split result slabs */
size_t rime_fringe_ant_bwd_workspace(int Nbl, int Nt, int Nf);              /* backward: transposed gvis */
int rime_fringe_ant_fwd(const double* antpos, const double* sdir, const double* freqs,
                        const float* psky, const float* scale, const float* rowmin,
                        const int* pair_direct,
                        const int* pair_conj, int Nant, int Nbl, int Nt, int Nf, int Pstride,
                        long long st_t, long long st_f, long long st_p, int sign, float* vis,
                        void* workspace, size_t workspace_bytes, void* stream);
int rime_fringe_ant_bwd(const double* antpos, const double* sdir, const double* freqs,
                        const float* gvis, const float* gscale, const int* pair_direct,
                        const int* pair_conj, int Nant, int Nbl, int Nt, int Nf, int Pstride,
                        long long st_t, long long st_f, long long st_p, int sign, float* gpsky,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Block decomposition of the pair matrix.  The antennas are cut into groups (<= 128 antennas: by
 * position for arrays with more than 128 antennas, by beam model when antennas carry different beam
 * models -- beam_model.py:303-327 pairs them per baseline --, by rank-local tile for baseline-tile
 * sharding across GPUs) and the pair matrix into blocks; every block is one launch with its own psky
 * plane.  rime_fringe_ant_fwd == one diagonal block + finish; rime_fringe_ant_bwd == prepare + one
 * diagonal block.
 *   diagonal block (cross = 0): antpos [Nrows <= 128, 3] of one group against itself, tables as above
 *       (local indices)
 *   cross block (cross = rows of group I): antpos [Nrows, 3] = group I (cross rows) then group J
 *       (Nrows - cross rows), each zero-padded to a multiple of 32; supported (rows I, rows J): (32, 32),
 *       (32, 64), (64, 64), (128, 128); pair_direct[i*128 + j] = slot of baseline (I_i -> J_j),
 *       pair_conj[i*128 + j] = slot of baseline (J_j -> I_i), or -1
 *   self block (forward only, cross == Nrows in {32, 64, 96, 128}, psky_complex != 0): the diagonal block of one
 *       group as the cross block of the group with ITSELF -- antpos [Nrows, 3] zero-padded, the tables of the
 *       diagonal block (entries i < j); L and B images of the same antennas come from one evaluation of the
 *       phase, only the upper-triangular tiles are contracted
 *   psky_complex: 0 = psky / gpsky is one real plane (st_p 1 or 2); +1 = interleaved complex (st_p == 2)
 *       handled in ONE pass (forward: cross and self blocks -- a diagonal block (cross = 0) returns
 *       RIME_EUNSUPPORTED and takes one call per real plane; the block must hold direct entries only); -1 = as +1 but the
 *       block contracts conj(psky) (a block built with its groups swapped: conj entries only).  The
 *       backward writes both gradient planes from one pass for either block kind.
 *   mirror: bit mask over the 16-row groups g of a DIAGONAL block (0 = none; round 5).  Bit g set: rows 16 g + 8 + i hold the
 *       MIRROR antennas of rows 16 g + i, i < 8 -- antpos[16 g + 8 + i] = -antpos[16 g + i] (the block's positions are
 *       measured from the centre of symmetry; visibilities depend on position differences only), rows without an antenna
 *       in either octet zero.  Their phasors are complex conjugates: the kernels evaluate the first octet and conjugate
 *       it for the second (forward: the real-plane passes of every diagonal block -- the 33..48-row shape in its first row
 *       tile only; backward: every diagonal block).  A licence, not an obligation: other block kinds evaluate every row.  Bits at or beyond ceil(Nrows / 16) -> RIME_EINVAL.
 * Forward blocks fill disjoint baseline slots of the slab workspace (every baseline must belong
 * to exactly one block); _finish sums the pixel splits and writes vis [Nbl, Nt, Nf].  Backward:
 * _prepare transposes gvis into the workspace once, every block reads it; blocks after the first that
 * write the same gpsky plane pass accumulate = 1 (stream order makes the sum deterministic). */
int rime_fringe_ant_fwd_block(const double* antpos, int Nrows, int cross, int mirror, const double* sdir,
                              const double* freqs, const float* psky, const float* scale,
                              const float* rowmin, const int* pair_direct, const int* pair_conj, int Nbl, int Nt, int Nf,
                              int Pstride, long long st_t, long long st_f, long long st_p, int sign,
                              int psky_complex, void* workspace, size_t workspace_bytes, void* stream);
/* Row pre-scales of the matrix-core kernels in one launch: for every row (i0, i1, i2, i3) of a 4-D arrangement of
 * contiguous float32 rows of length L at x + i0 s0 + i1 s1 + i2 s2 + i3 s3 (element strides):
 *   scale[row]  = 2^floor(log2(2^14 / max|x|)) (1 for an all-zero row)   -- the `scale` / `gscale` inputs above
 *   rowmin[row] = min x (or NULL)                                          -- the `rowmin` input of the forward
 * rows numbered ((i0 d1 + i1) d2 + i2) d3 + i3.  Host-side convenience (what the shipped binding computes these two
 * inputs with); the reference has no counterpart. */
int rime_fringe_row_scale(const float* x, int d0, int d1, int d2, int d3, long long s0, long long s1,
                          long long s2, long long s3, int L, float* scale, float* rowmin, void* stream);
/* The same for rows of an INTERLEAVED COMPLEX float32 psky (full-polarisation layouts; strides and L in complex elements):
 * scale[row] from max(|re|, |im|) over the row, rowmin_re / rowmin_im (or NULL) the minimum of each plane -- the `rowmin`
 * inputs of the per-plane forward passes. */
int rime_fringe_row_scale_cplx(const float* x, int d0, int d1, int d2, int d3, long long s0, long long s1,
                               long long s2, long long s3, int L, float* scale, float* rowmin_re, float* rowmin_im,
                               void* stream);
int rime_fringe_ant_fwd_finish(const void* workspace, size_t workspace_bytes, float* vis,
                               int Nbl, int Nt, int Nf, int Pstride, void* stream);
int rime_fringe_ant_bwd_prepare(const float* gvis, int Nbl, int Nt, int Nf,
                                void* workspace, size_t workspace_bytes, void* stream);
int rime_fringe_ant_bwd_block(const double* antpos, int Nrows, int cross, int mirror, const double* sdir,
                              const double* freqs, const float* gscale, const int* pair_direct,
                              const int* pair_conj, int Nbl, int Nt, int Nf, int Pstride,
                              long long st_t, long long st_f, long long st_p, int sign,
                              int psky_complex, int accumulate, float* gpsky, const void* workspace,
                              size_t workspace_bytes, void* stream);

/* Conjugate-pair form of a diagonal block, real psky (round 5; csrc/fringe_mfma.hip, "CONJUGATE-PAIR FORM").  Replaces the same
 * reference lines as the blocks above (telescope_model.py:310-358 + rime_model.py:423-429) for an array with POINT SYMMETRY:
 * antennas that come in mirror pairs about a centre c, r' - c = -(r - c), have conjugate phasors, and all pairs of up to
 * 128 (+ 1) antennas follow from the phasors of one antenna of each pair.
 *   antpos [Nrows <= 64, 3]: positions MEASURED FROM c of the "firsts" -- one antenna of every mirror pair -- and of the
 *       antennas without a partner, one per row.
 *   pair_direct / pair_conj: the tables of a VIRTUAL diagonal block of 128 rows -- row i < 64 = the antenna of antpos row i,
 *       row 64 + i = its mirror antenna (no antenna: no entries) -- built by the rule of every diagonal block
 *       (pair_direct[i*128 + j] = slot of baseline i -> j for tile(i) <= tile(j), else pair_conj[j*128 + i]).
 *   centre: NULL, or int32 [2][128] for ONE more antenna that sits at c itself (its phasor is 1; needed when the firsts and
 *       singles already fill 64 rows): centre[r] = slot of the baseline (hub -> virtual row r), centre[128 + r] = slot of
 *       (virtual row r -> hub), or -1.
 *   flat: nonzero = every antpos z is zero (a coplanar array measured from a centre in its plane): the kernels do not evaluate that
 *       term of the phase.  A licence stated by the caller; 0 is always correct.
 *   psky / gpsky is ONE real plane (st_p = 1, or 2 for a plane of an interleaved complex buffer: V is linear in psky, a complex
 *   psky takes one call per plane as on every diagonal block); the other arguments, the workspace and _finish / _prepare are those of rime_fringe_ant_fwd_block /
 *   rime_fringe_ant_bwd_block, and pair blocks mix with other blocks of the same launch sequence. */
int rime_fringe_pair_fwd_block(const double* antpos, int Nrows, const int* centre, int flat, const double* sdir,
                               const double* freqs, const float* psky, const float* scale, const float* rowmin,
                               const int* pair_direct, const int* pair_conj, int Nbl, int Nt, int Nf, int Pstride,
                               long long st_t, long long st_f, long long st_p, int sign,
                               void* workspace, size_t workspace_bytes, void* stream);
int rime_fringe_pair_bwd_block(const double* antpos, int Nrows, const int* centre, int flat, const double* sdir,
                               const double* freqs, const float* gscale, const int* pair_direct,
                               const int* pair_conj, int Nbl, int Nt, int Nf, int Pstride,
                               long long st_t, long long st_f, long long st_p, int sign, int accumulate,
                               float* gpsky, const void* workspace, size_t workspace_bytes, void* stream);
/* Pixel splits of a rime_fringe_pair_bwd_block launch (blocks = Nt x splits x Nf): 256 pixel tiles of 32 per block, fewer on
 * a small grid, up to 1024 where at least 6144 blocks remain (every block stages the G planes of its row anew).  0 for a
 * shape the block entry refuses.  RIME_PAIR_BWD_WIDE=0 (A/B measurements) keeps 256 at most; the answer is the plan in
 * force.  Host only. */
int rime_fringe_pair_bwd_splits(int Nt, int Nf, int Pstride);

/* SEGMENTS: the pair blocks of up to 4 psky planes that share rows, slot tables, times and channels -- the sky components of
 * one RIME call -- in ONE launch per direction.  A segment names what a plane has of its own; the fields of the other
 * direction are ignored.  rime_fringe_pair_fwd_block / rime_fringe_pair_bwd_block are these entry points with one segment. */
typedef struct rime_fringe_segment {
    const double* sdir;          /* [Nt, 3, Pstride] */
    const float* psky;           /* forward: the plane, strided [t][f][p] */
    const float* scale;          /* forward: [Nt, Nf] power-of-two pre-scale of its rows */
    const float* rowmin;         /* forward: [Nt, Nf] row minima, or NULL (every row signed) */
    float* gpsky;                /* backward: the gradient plane, same strides */
    long long st_t, st_f, st_p;  /* element strides; st_p 1 or 2 */
    int Pstride;                 /* multiple of 64 */
    int accumulate;              /* backward: add to gpsky */
} rime_fringe_segment;
/* Forward: the slabs of segment k follow those of segments 0 .. k - 1 in the workspace (_segments_workspace bytes; 0 for a
 * refused shape) and _segments_finish sums all of them into vis in that order, splits of a segment in split order: the bits of
 * per-plane launches, finished one by one and added, whenever every segment after the first has one split.  In the GRID the
 * segment with the most pixels stands first.  Backward: `workspace` is what rime_fringe_ant_bwd_prepare wrote, gscale the
 * scale of its rows; a segment's pixel split widens by the rule of rime_fringe_pair_bwd_splits with the block count of ALL
 * segments (pixel tiles are independent outputs: the same bits for every split).
 * _segments_map (host only): the grid size, and with out != NULL ([grid][6] ints, capacity in blocks) for every block its
 * (segment, f, t, split, first, end) -- panels (forward) or pixel tiles (backward) of 32 pixels -- as the kernels resolve it. */
size_t rime_fringe_pair_segments_workspace(int Nbl, int Nt, int Nf, const int* Pstride, int nseg);
int rime_fringe_pair_segments_map(int backward, int Nt, int Nf, const int* Pstride, int nseg, int* out, long capacity);
int rime_fringe_pair_fwd_segments(const double* antpos, int Nrows, const int* centre, int flat, const double* freqs,
                                  const int* pair_direct, const int* pair_conj, int Nbl, int Nt, int Nf, int sign,
                                  const rime_fringe_segment* segs, int nseg, void* workspace, size_t workspace_bytes,
                                  void* stream);
int rime_fringe_pair_segments_finish(const void* workspace, size_t workspace_bytes, float* vis, int Nbl, int Nt, int Nf,
                                     const int* Pstride, int nseg, void* stream);
int rime_fringe_pair_bwd_segments(const double* antpos, int Nrows, const int* centre, int flat, const double* freqs,
                                  const float* gscale, const int* pair_direct, const int* pair_conj, int Nbl, int Nt,
                                  int Nf, int sign, const rime_fringe_segment* segs, int nseg, const void* workspace,
                                  size_t workspace_bytes, void* stream);

/* Conjugate-pair CROSS block, real psky (csrc/fringe_xpair.hip): the block between two groups I and J of ONE point-symmetric
 * array with more than 128 antennas.  Both groups are closed under the mirror (a group is a set of rows together with their
 * mirror antennas) and are measured from the SAME centre c, so the four quadrants V[x, y], V[x', y'], V[x', y], V[x, y'] follow
 * from four real products of the rows' images: 48 MFMAs per 16 pixels instead of the 192 of a generic (128, 128) cross block,
 * from rows_i + rows_j generated rows instead of twice as many.
 *   antpos [rows_i + rows_j, 3]: positions measured from c of the rows of group I, then of group J (1 <= rows <= 64 each); a
 *       row is one antenna of a mirror pair, an antenna without a partner, or the antenna at c itself (position 0).
 *   pair_direct / pair_conj [128 * 128]: r = k for the antenna of row k of I, 64 + k for its mirror; c = l for the antenna of
 *       row l of J, 64 + l for its mirror.  pair_direct[r*128 + c] = slot of the baseline r -> c (receives V[r, c]),
 *       pair_conj[r*128 + c] = slot of the baseline c -> r (receives its conjugate), or -1.  A row without a mirror has no
 *       entries in its mirror quadrants.
 *   flat: as for the pair blocks.  psky / gpsky is ONE real plane (st_p = 1, or 2: a plane of an interleaved complex buffer).
 * The other arguments, the workspace and _finish / _prepare are those of rime_fringe_pair_fwd_block / rime_fringe_pair_bwd_block;
 * the blocks mix with every other block kind in one launch sequence.  -1 on a bad argument, -2 on a short workspace. */
int rime_fringe_pair_cross_fwd_block(const double* antpos, int rows_i, int rows_j, int flat, const double* sdir,
                                     const double* freqs, const float* psky, const float* scale, const float* rowmin,
                                     const int* pair_direct, const int* pair_conj, int Nbl, int Nt, int Nf, int Pstride,
                                     long long st_t, long long st_f, long long st_p, int sign,
                                     void* workspace, size_t workspace_bytes, void* stream);
int rime_fringe_pair_cross_bwd_block(const double* antpos, int rows_i, int rows_j, int flat, const double* sdir,
                                     const double* freqs, const float* gscale, const int* pair_direct,
                                     const int* pair_conj, int Nbl, int Nt, int Nf, int Pstride,
                                     long long st_t, long long st_f, long long st_p, int sign, int accumulate,
                                     float* gpsky, const void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * ICRS (ra, dec) -> topocentric (zenith angle, azimuth East of North), degrees, float64.
 * Replaces the per-direction part of telescope_model.eq2top (telescope_model.py:469-502,
 * astropy ICRS -> AltAz): annual aberration, rotation by the caller's 3 x 3 matrix
 * M = L(lat) R3(GAST + lon) N P B (ICRS -> East, North, Up; bayeslim_amd/astrometry.py builds it
 * per observation time: IAU 2006 precession + frame bias, truncated IAU 1980 nutation, GAST),
 * diurnal aberration, conversion to angles.
 *   ra_deg, dec_deg, zen_deg, az_deg: device f64 [N];  M_host f64 [9] row-major and
 *   vbary_host f64 [3] (observer velocity / c, ICRS axes) are HOST pointers; vdiurnal = eastward
 *   site velocity / c
 * ------------------------------------------------------------------------------------- */
int rime_eq2top(const double* ra_deg, const double* dec_deg, int N, const double* M_host,
                const double* vbary_host, double vdiurnal, double* zen_deg, double* az_deg, void* stream);

/* ---------------------------------------------------------------------------------------
 * Materialised fringe, for callers that want the tensor itself (imaging.VisMapper.build_A,
 * tests):  out[b, f, p] = exp(sign * 2 pi i * freqs[f]/c * blvecs[b] . sdir[:, p])
 * Replaces ArrayModel.gen_fringe (telescope_model.py:350-356).  RIME never calls it.
 *   sdir f64 [3, sdir_stride];  out complex<T> [Nbl, Nf, P]
 * ------------------------------------------------------------------------------------- */
int rime_gen_fringe(int dtype, const double* blvecs, const double* sdir, const double* freqs,
                    int Nbl, int Nf, int P, int sdir_stride, int sign, void* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Pixel-beam interpolation gather:  out[r, p] = sum_k wgts[p, k] * m[r, inds[p, k]]
 * Replaces PixInterp.interp (utils.py:815-861: index_select + einsum).
 *   m    T [R, Npb]   (R = product of leading dims: Npol*Nvec*Nmodel*Nf), or complex<T>
 *   inds int32 [P, Nnn];  wgts T [P, Nnn];  out T [R, out_stride] (columns >= P untouched)
 * ------------------------------------------------------------------------------------- */
int rime_interp_gather_fwd(int dtype, int is_complex, const void* m, const int* inds,
                           const void* wgts, int R, int Npb, int P, int Nnn,
                           void* out, int out_stride, void* stream);

/* Adjoint of the gather, deterministic: gm[r, j] = sum over (p,k) with inds[p,k]==j of
 * wgts[p,k] * gout[r, p], driven by a CSR inverse index built once per (inds, wgts):
 *   csr_ptr int32 [Npb+1], csr_src int32 [nnz] (flat p*Nnn+k positions, ascending per row).
 * Both tensors are passed TRANSPOSED so that every access is coalesced:
 *   goutT T [P, R] (complex: [P, R, 2]) -- all map rows of one sky pixel contiguous
 *   gmT   T [Npb, R] (complex: [Npb, R, 2])
 * Replaces the index_select/einsum backward (scatter-add) of utils.py:833-841. */
int rime_interp_scatter_bwd(int dtype, int is_complex, const void* goutT,
                            const int* csr_ptr, const int* csr_src, const void* wgts,
                            int R, int Npb, int P, int Nnn, void* gmT, void* stream);
/* The same adjoint for a ONE-NODE stencil (Nnn = 1: the FoV cut, cut_sky_fov beam_model.py:1681-1698, and the redundant
 * inflation, rime_model.py:436-437) on ROW-MAJOR buffers -- no transposed copies:
 *   gout T [R, gout_stride] (complex: [R, gout_stride, 2]), gm T [R, Npb]; csr_src holds point indices q, wgts T [P].
 *   Any R (rows beyond one grid's reach take further launches); an EMPTY index (csr_ptr all zero: every weight 0) may pass
 *   csr_src = NULL and yields gm = 0. */
int rime_interp_scatter_rows_bwd(int dtype, int is_complex, const void* gout, long long gout_stride,
                                 const int* csr_ptr, const int* csr_src, const void* wgts, int R, int Npb,
                                 void* gm, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused psky builder (1-pol power beam, one beam model):
 *   psky[r, q] = ( sum_k wgts[q,k] * bmapT[inds[q,k], r] ) * sky[r, cut[q]],  r = channel, q = (t, p)
 * = PixelBeam.gen_beam's interpolation (beam_model.py:238-269) + cut_sky_fov (:1681-1698) + the
 * beam x sky product of apply_beam (:313-322) in one pass; cut[q] == Npix marks zero padding.
 *   bmapT T [Npb, R] (the beam map NODE-MAJOR: a node's channels are contiguous, so the gathers are vector
 *   loads); sky T [R, Npix]; inds i32 / wgts T [Q = Nt*Ps, Nnn]; cut i32 [Q]; psky T [R, Q]
 * Backward: T1 [Q, R] = gpsky * sky_cut (transposed: the input layout of rime_interp_scatter_bwd, which
 * then yields the beam-map gradient); gsky [R, Npix] = sum over time steps of gpsky * (re-interpolated beam)
 * through pos i32 [Nt, Npix] (index of sky pixel j inside time step t's cut, or -1).  No atomics.
 * ------------------------------------------------------------------------------------- */
int rime_beam_sky_fwd(int dtype, const void* bmapT, const void* sky, const int* inds, const void* wgts,
                      const int* cut, int R, int Npb, int Npix, int Q, int Nnn, void* psky, void* stream);
/* workspace: partial planes of the sky gradient when its time steps are split over blocks (workloads of many time steps and
 * few sky pixels; 0 bytes when one block walks all steps).  NULL = no split. */
size_t rime_beam_sky_bwd_workspace(int dtype, int R, int Npix, int Nt);
int rime_beam_sky_bwd(int dtype, const void* gpsky, const void* bmapT, const void* sky, const int* inds,
                      const void* wgts, const int* cut, const int* pos, int R, int Npb, int Npix,
                      int Nt, int Ps, int Nnn, void* T1, void* gsky, void* workspace, size_t workspace_bytes,
                      void* stream);

/* ---------------------------------------------------------------------------------------
 * Full-polarisation beam x sky product, elementwise:  psky[a, d] = sum_{b, c} J1[a, b] S[b, c] conj(J2[d, c])
 * Replaces the 4-pol branch of PixelBeam.apply_beam (beam_model.py:345-363, einsum "ab...,bc...,dc...->ad...") and
 * its autograd backward in one pass each (the torch composition materialises two temporaries of 8 x psky).
 *   J1, J2 : T [2, 2, N] (beam_complex = 0) or complex<T> [2, 2, N];  J2 may be the same pointer as J1
 *   S      : complex<T> [2, 2, Ns], Ns dividing N (one sky for all Nmp model pairs: element n reads n % Ns)
 *   out, G : complex<T> [2, 2, N]  (N = Nmp * Nf * P)
 * Backward: gS [2, 2, N] = J1^H G J2 (the caller sums over model pairs when Ns < N), gJ1 = G (S J2^H)^H,
 * gJ2 = G^H (J1 S) -- real parts for a real beam -- each [2, 2, N] in the beam's type.  The caller adds gJ1 + gJ2 when
 * J2 is J1.
 * ------------------------------------------------------------------------------------- */
int rime_jones_apply_fwd(int dtype, int beam_complex, const void* J1, const void* J2, const void* S,
                         long long N, long long Ns, void* out, void* stream);
int rime_jones_apply_bwd(int dtype, int beam_complex, const void* J1, const void* J2, const void* S,
                         const void* G, long long N, long long Ns, void* gJ1, void* gJ2, void* gS, void* stream);

/* Stokes I + fractional polarisation -> coherency matrix, one pass each way
 *   C = I [[1 + fQ, fU - i fV], [fU + i fV, 1 - fQ]]
 * (sky_model.py:1160-1300: Stokes2Coherency on a Stokes-I sky with fractions; the reference composes it from ~15 tensor ops).
 *   stokesI : T [R, P] contiguous;  frac : T, element f_k[r, p] at frac[k fs_k + r fs_r + p fs_p] (strides 0 = broadcast), k = Q, U, V
 *   coh, gcoh : complex<T> [2, 2, R, P];   gI : T [R, P] = (1 + fQ) Re g00 + (1 - fQ) Re g11 + fU (Re g01 + Re g10) + fV (Im g10 - Im g01) */
int rime_stokes2coh_fwd(int dtype, const void* stokesI, const void* frac, long long fs_k, long long fs_r, long long fs_p,
                        long long R, long long P, void* coh, void* stream);
int rime_stokes2coh_bwd(int dtype, const void* gcoh, const void* frac, long long fs_k, long long fs_r, long long fs_p,
                        long long R, long long P, void* gI, void* stream);

/* ---------------------------------------------------------------------------------------
 * a_lm -> pixel transform:  out[r, j] = sum_c ( are[r,c] * Yre[c,j] - aim[r,c] * Yim[c,j] )
 *   = Re( (a * alm_mult) @ Ylm ), with alm_mult already folded into `alm` by the caller
 *   (an elementwise torch op, kept in autograd).
 * Replaces AlmModel.forward_alm (sph_harm.py:1342-1372), real_output=True branch.
 *   alm  T [R, Ncoeff, 2] (interleaved complex);  Ylm T [Ncoeff, Npix, 2];  out T [R, Npix]
 * Backward: galm[r, c] = sum_j gout[r, j] * conj(Ylm[c, j])   (complex, interleaved); the pixel
 *   axis may be split over blocks, partial sums go to a caller-owned workspace
 *   (rime_alm2pix_bwd_workspace bytes) and are reduced deterministically.
 * float32, y_scale > 0: operands split into f16 hi + lo halves on v_mfma_f32_32x32x16_f16 (three
 *   cross products, f32 accumulation, 22 significant bits) so both directions run at the rate Ylm
 *   streams from HBM.  y_scale is a power of two that brings max|Ylm| into [2^10, 2^14] (1.0 for
 *   orthonormal Ylm); the row operand is scaled per row inside the library.
 * float32, y_scale == 0: exact-f32 matrix cores (v_mfma_f32_32x32x2_f32).  float64: VALU.
 * Both directions take a caller-owned workspace (rime_alm2pix_*_workspace bytes).
 * ------------------------------------------------------------------------------------- */
size_t rime_alm2pix_fwd_workspace(int dtype, int R, int Ncoeff, int Npix);
int rime_alm2pix_fwd(int dtype, const void* alm, const void* Ylm, double y_scale, int R, int Ncoeff,
                     int Npix, void* out, void* workspace, size_t workspace_bytes, void* stream);
size_t rime_alm2pix_bwd_workspace(int dtype, int R, int Ncoeff, int Npix);
int rime_alm2pix_bwd(int dtype, const void* gout, const void* Ylm, double y_scale, int R, int Ncoeff,
                     int Npix, void* galm, void* workspace, size_t workspace_bytes, void* stream);

/* Packed Ylm (float32 f16-split path only): Ylm x y_scale split ONCE into f16 hi / lo halves, stored in the order the
 * matrix-core fragments are consumed -- 8 bytes per (coefficient, pixel), as the complex64 matrix itself, one copy per
 * direction (0 = forward: contraction over coefficients; 1 = backward: contraction over pixels).  The transforms on a
 * packed copy do no arithmetic on the streamed operand and read it as fully coalesced 1-KB fragments; the products are
 * those of rime_alm2pix_fwd / _bwd with y_scale > 0 (same split, same MFMAs): the forward is bitwise equal (same summation
 * order over K) as long as it runs WITHOUT a K split -- maps that offer fewer 4-wave blocks than 1.5 resident grids (the C3
 * shape: 2 splits) sum two partial planes in a second kernel, another order of the float32 sums (~2e-6 of the maximum) --, the backward
 * differs in the order of its float32 partial sums over pixels (~1e-6).  The caller owns the packed buffer (rime_alm2pix_packed_bytes) and must pack
 * again when Ylm or y_scale changes.  Workspaces: rime_alm2pix_fwd_workspace / rime_alm2pix_bwd_workspace bytes.
 * Same reference lines as above (sph_harm.py:1342-1372); the reference recomputes the einsum on the complex matrix. */
size_t rime_alm2pix_packed_bytes(int Ncoeff, int Npix, int direction);
int rime_alm2pix_pack(const void* Ylm, double y_scale, int Ncoeff, int Npix, int direction, void* packed, void* stream);
int rime_alm2pix_fwd_packed(const void* alm, const void* packed, double y_scale, int R, int Ncoeff, int Npix,
                            void* out, void* workspace, size_t workspace_bytes, void* stream);
int rime_alm2pix_bwd_packed(const void* gout, const void* packed, double y_scale, int R, int Ncoeff, int Npix,
                            void* galm, void* workspace, size_t workspace_bytes, void* stream);

/* The plan in force for one transform: which kernel family the entry point above would launch for these arguments and on
 * what grid.  `direction` 0 = forward, 1 = backward; `packed` 1 = rime_alm2pix_fwd_packed / _bwd_packed (float32 and
 * y_scale > 0 only), 0 = rime_alm2pix_fwd / _bwd.  Fills plan[0 .. 5]:
 *   plan[0] kernel family (RIME_ALM_*, below)
 *   plan[1] MT: row tiles of 32 per block (1, 2 or 4; 0 for the float64 VALU kernels)
 *   plan[2] row tiles of the grid (blocks along the rows)
 *   plan[3] column tiles of the grid (blocks along the pixels in the forward, along the coefficients in the backward)
 *   plan[4] S: pixel splits of the backward / K splits of the packed forward (1 = no partial planes, no reduction)
 *   plan[5] 1 when the row operand takes the tiled long-row split (f16-split families), else 0
 * Answered by the functions the launches themselves call, the switches RIME_ALM_BWD_DMA, RIME_ALM_BWD_WIDE (read once
 * per process), RIME_ALM_BWD_SPLITS and RIME_ALM_FWD_SPLITS (read on every call) included.  Host only: no launch, no
 * allocation.  RIME_EINVAL for a null plan, an unknown dtype, a negative or NaN y_scale, an extent <= 0, a direction or
 * packed flag outside {0, 1}, and packed = 1 with float64 or y_scale == 0. */
#define RIME_ALM_F64_VALU 0   /* float64, vector ALU                                                        */
#define RIME_ALM_F32_MFMA 1   /* float32, y_scale == 0: exact-f32 matrix cores                              */
#define RIME_ALM_F16_REG  2   /* f16 split, Ylm staged through registers (forward; backward at odd Npix)    */
#define RIME_ALM_F16_DMA  3   /* f16 split, backward: LDS-DMA ring (even Npix)                              */
#define RIME_ALM_PACKED4  4   /* packed Ylm, 4-wave blocks                                                  */
#define RIME_ALM_PACKED8  5   /* packed Ylm, backward above 64 rows: 8-wave blocks of 256 coefficients      */
int rime_alm2pix_plan(int dtype, double y_scale, int R, int Ncoeff, int Npix, int direction, int packed, int* plan);

/* ---------------------------------------------------------------------------------------
 * Spherical Fourier-Bessel radial transform  a_lm(r) = sum_n g_l(k_ln r) t_lmn  for every degree l in ONE launch
 * (SFBModel.forward_gln, sph_harm.py:1979-1982: a Python loop of one small matmul per degree) and its adjoint.
 *   forward   out[b, r, cols[col_off + c]] = sum_n g[g_off + n Nr + r] * params[b, p_off + n Nl + c]
 *   backward  gparams[b, p_off + n Nl + c] = sum_r g[g_off + n Nr + r] * gout[b, r, cols[col_off + c]]
 *   params / gparams T [B, Nlmn] (x2 interleaved re, im when cplx = 1); out / gout T [B, Nr, Nlm] (x2 when cplx);
 *   g T: the real (Nk, Nr) matrices of all degrees packed one after another, row n of a degree contiguous in r;
 *   blocks int32 [Nblk][5] = (g_off, Nk, p_off, col_off, Nl) per degree; cols int32: the a_lm columns of every degree,
 *   a degree's Nl entries starting at col_off; tiles int32 [Ntile][3] = (block, i0, c0): a 64 x 32 tile of the
 *   (Nr x Nl) output of a degree forwards (i0 a multiple of 64 in r), of its (Nk x Nl) parameter block backwards
 *   (i0 a multiple of 64 in n), c0 a multiple of 32.  One work-group per tile and batch row; the forward list holds
 *   tiles for degrees with Nk = 0 too (their columns are stored as zeros), the backward list needs none for them.
 * Every element covered by a tile is written exactly once (no atomics, no zero-fill, sums in ascending order:
 * bit-reproducible); out columns that belong to no degree are NOT written -- the caller zero-fills when its tables
 * do not cover all Nlm columns.  The parameter blocks partition [0, Nlmn), so gparams is fully defined.
 * No gradient with respect to g.  Accumulation in T.  Ntile = 0 or B = 0 returns RIME_OK without a launch.
 * ------------------------------------------------------------------------------------- */
int rime_sfb_fwd(int dtype, int cplx, const void* params, const void* g, const int* blocks, const int* cols,
                 const int* tiles, int Nblk, int Ntile, int B, int Nlmn, int Nr, int Nlm, void* out, void* stream);
int rime_sfb_bwd(int dtype, int cplx, const void* gout, const void* g, const int* blocks, const int* cols,
                 const int* tiles, int Nblk, int Ntile, int B, int Nlmn, int Nr, int Nlm, void* gparams, void* stream);

/* ---------------------------------------------------------------------------------------
 * Grouped matrix filter along the last axis of a complex tensor: the reference's MatFilter / GPFilter / WedgeFilter
 * (filt.py:89-160, 382-397: per baseline group a gather, a complex einsum and a scatter) in ONE launch, forward and adjoint.
 * For every line l (Nx contiguous complex samples of x, Ny of y) with filter index f(l):
 *     acc_i       = sum_k W[f(l)][i, k] * x[l, ic[k]]                  i < M, k < K
 *     y[l, oc[i]] = s * acc_i + base[i] * x[l, oc[i]]
 *   x T [Nlines][Nx][2], y T [Nlines][Ny][2] (interleaved re, im); ic int32 [K] (columns of x), oc int32 [M] (columns of y,
 *   and of x where base[i] != 0), base T [M]; s = +1 or -1.
 *   Wt T [Nfilt][KR][M], the filters TRANSPOSED (contraction index major): wcplx = 0: KR = K, Wt[f][k][i] = W[f][i][k];
 *   wcplx = 1: KR = 2K, Wt[f][2k][i] = Re W[f][i][k], Wt[f][2k+1][i] = -Im W[f][i][k].
 *   tiles int32 [Ntile][65] = (filter, 64 line indices, -1 = padding): the host groups the lines by filter.  A tile of
 *   filter -1 copies its lines from x to y; Npass is the number of such tiles and Nx == Ny is required when Npass > 0.
 *   One work-group per tile and per 128 output rows.  Every (line, oc[i]) of a listed line is written exactly once; no other
 *   element of y is touched (the caller provides them); no atomics, sums in ascending k: bit-reproducible.
 * float32 runs on v_mfma_f32_32x32x2_f32 (an exact fmaf chain), float64 on the vector ALU.  Forward: W = G, ic the identity,
 * oc = input_idx or the identity, base = residual, s = residual ? -1 : +1.  Adjoint: W = G^H, ic = input_idx, oc the identity.
 * No gradient with respect to W.  Ntile = 0 or Nlines = 0 returns RIME_OK without a launch.
 * ------------------------------------------------------------------------------------- */
int rime_filt_apply(int dtype, int wcplx, const void* x, const void* Wt, const int* ic, const int* oc, const void* base,
                    const int* tiles, int Ntile, int Npass, int Nfilt, int M, int K, int Nx, int Ny, long long Nlines,
                    double s, void* y, void* stream);

/* ---------------------------------------------------------------------------------------
 * Batched 1-D complex DFT along the last axis with the reference's FFT block fused around it (fft.py:99-202: window,
 * ifftshift, fft, fftshift, abs, peak normalisation, |.|^2, and PeakDelay's per-line Quinn estimate) in ONE launch.
 * For every line l of N interleaved complex samples, 1 <= N <= 4096:
 *     X[k]   = wl[src] x[l, src],  src = (k + shift_in) mod N             (wl = win when win_on_store = 0, else 1)
 *     Y      = sum_k X[k] tw[(j k) mod N]                                 tw T [N][2] = exp(-+2 pi i j / N), caller-built
 *     z[k]   = ws[k] scale Y[(k + shift_out) mod N]                       (ws = win when win_on_store = 1, else 1)
 *     y[l,k] = epilogue(z[k])
 *   radix int32 [nradix], HOST memory: the Stockham pass radices, product N (2, 3, 4, 5 are written out, any other radix
 *   runs as r-term sums); inverse (0 / 1) names the sign of tw's exponent (0: minus); win T [N] real or NULL.
 *   epilogue: a sum of RIME_FFT_ABS (1), RIME_FFT_PEAKNORM (2, divide by the line's max |z|), RIME_FFT_SQUARE (4), applied in
 *   that order as the reference does; y is T [nlines][N][2] for 0 and 2, T [nlines][N] real when 1 or 4 is set.  With
 *   RIME_FFT_PEAK (8) added y is T [nlines]: start + (n + delta) df with n the first index of the maximum of |z| and delta
 *   Quinn's second estimator from the epilogue's values at n - 1, n, n + 1 (indices wrap round).
 * The adjoint of a call (epilogue 0) is the call with inverse flipped and the other table, shift_in' = (N - shift_out) mod N,
 * shift_out' = (N - shift_in) mod N, win_on_store flipped and the same scale.
 * One work-group per 1024 / N lines (one above 512 samples); every output is written exactly once, no atomics, sums in a
 * fixed order: bit-reproducible.  All arguments are checked before any HIP call: RIME_EINVAL for N < 1, N > 4096, an
 * unknown dtype or epilogue, a null x / y / tw, a radix list whose product is not N, a shift outside [0, N).
 * nlines = 0 returns RIME_OK without a launch.
 * ------------------------------------------------------------------------------------- */
#define RIME_FFT_ABS 1
#define RIME_FFT_PEAKNORM 2
#define RIME_FFT_SQUARE 4
#define RIME_FFT_PEAK 8
int rime_fft_apply(int dtype, const void* x, const void* tw, const void* win, int win_on_store, const int* radix,
                   int nradix, int N, long long nlines, int inverse, int shift_in, int shift_out, double scale,
                   int epilogue, double start, double df, void* y, void* stream);

/* ---------------------------------------------------------------------------------------
 * Linear model along a middle axis: the reference's LinearModel.forward (linear_model.py:121-169: params * coeff,
 * index_select, matmul or einsum, .real) in ONE launch, and the same launch with M = A^H for its backward pass and for the
 * A^H y product of least squares.  For a contiguous x [O][K_in][I] and a matrix M [R][K]:
 *     y[o, r, i] = post[r] * sum_{k < K} M[r, k] * pre[k] * x[o, idx[k], i]              y [O][R][I] contiguous
 *   x: T (xcplx = 0) or interleaved complex T (xcplx = 1); M likewise (mcplx), element (r, k) at element offset
 *   r * m_rs + k * m_ks (both > 0; the kernels walk k fastest when I > 1 and K <= 32, r fastest otherwise: store M so that
 *   this index is contiguous); y is complex when x or M is, unless out_real = 1: then only Re(M x) = Mr xr - Mi xi is
 *   computed and y is real.  out_real needs a complex x: for a real x the caller passes Re(M).
 *   idx int32 [K] (device): rows of x along the contracted axis, each in [0, K_in), repeats allowed; NULL: the identity, and
 *   K_in must equal K.  The kernel does not check the entries of idx.  pre T [K], post T [R]: real scalings, or NULL.
 * Forward: M = A, pre = coeff[idx], idx.  Adjoint: M = A^H, post = coeff[idx], no idx; the caller scatters the compact
 * [O][K][I] result through idx.  I > 1 runs one lane per column (o, i): with K <= 32 the K inputs of a column stay in
 * registers and the rows are looped over, with K > 32 up to 32 rows are accumulated in registers (R > 32 is tiled by 32 over the
 * grid and x re-read per tile); I == 1 runs lanes along r with M and the lines
 * staged in LDS.  Every output is written exactly once, sums in ascending k, no atomics: bit-reproducible.  No workspace.
 * All arguments are checked before any HIP call: RIME_EINVAL for an unknown dtype or flag, K, R, O or I <= 0, a null x, M
 * or y, out_real with a real x, idx with K_in <= 0, no idx with K_in != K, a stride <= 0, O * max(K_in, R) * I >= 2^62.
 * ------------------------------------------------------------------------------------- */
int rime_lm_apply(int dtype, int xcplx, int mcplx, int out_real, const void* x, const void* M, long long m_rs,
                  long long m_ks, const int* idx, const void* pre, const void* post, long long O, int K, int K_in,
                  int R, long long I, void* y, void* stream);

/* ---------------------------------------------------------------------------------------
 * Likelihood epilogue:  chi^2 = sum_i icov[i] * |pred[i] - data[i]|^2  over a complex visibility tensor
 * (N complex elements, interleaved), and its backward gpred[i] = 2 g icov[i] (pred[i] - data[i]).
 * Replaces `res = prediction - data; apply_icov(res, icov, cov_axis=None); torch.sum(...)` of
 * LogProb.forward_chisq (optim.py:1019-1027, apply_icov :1889-1894) -- SURVEY section 8(f) item 4.
 *   data NULL -> 0; icov T [N] real or NULL -> 1; out T [1]; g T [1] (device scalar: upstream gradient)
 * Deterministic two-pass reduction (double partial sums in a caller-owned workspace).
 * ------------------------------------------------------------------------------------- */
size_t rime_chisq_workspace(void);
int rime_chisq_fwd(int dtype, const void* pred, const void* data, const void* icov, size_t N,
                   void* out, void* workspace, size_t workspace_bytes, void* stream);
int rime_chisq_bwd(int dtype, const void* pred, const void* data, const void* icov, const void* g,
                   size_t N, void* gpred, void* stream);

/* ---------------------------------------------------------------------------------------
 * Log-priors over a real parameter tensor x of N elements (optim.LogLaplacePrior, optim.LogTaperedUniformPrior): out = sum_i t(x_i)
 * and, in the same pass, dx[i] = dt/dx_i, so that the backward is gx = g[0] dx (rime_prior_bwd).
 *   kind 0 laplace        t = -|r| / s, r = x - m; side 0 both, 1 upper (r < 0 -> 0), 2 lower (r > 0 -> 0);  d = -sign(r) / s
 *   kind 1 taper_sigmoid  t = logsig(c (x - l)) + logsig(-c (x - u)),  logsig(z) = min(z, 0) - log1p(exp(-|z|))
 *   kind 2 taper_tanh     t = log tanh(c (x - l)) + log tanh(-c (x - u));  NaN outside a bound
 *   m, s, l, u, c: T, each with a period: 1 one scalar, N a full tensor, 1 < period < N dividing N: element i % period
 *   (an operand shaped as the trailing axes of x).  NULL l or u: that term is dropped.  x, full operands, dx, gx: aligned to
 *   sizeof(T); 16-byte aligned ones take 16-byte accesses, the result does not depend on it.
 *   out T [1]; dx T [N] or NULL (not wanted: nothing is stored); g T [1] (device scalar: upstream gradient)
 * Deterministic two-pass reduction (double partial sums in a caller-owned workspace of rime_prior_workspace bytes).
 * RIME_EINVAL before any launch: null x / out (dx / g / gx), N == 0, unknown dtype / kind / side, a period of a given operand
 * that is 0, above N, or between 1 and N without dividing N, laplace without m and s, a taper without l and u or without c;
 * RIME_EWORKSPACE after these.
 * ------------------------------------------------------------------------------------- */
size_t rime_prior_workspace(void);
int rime_prior_fwd(int dtype, int kind, int side, const void* x, size_t N, const void* m, size_t m_period,
                   const void* s, size_t s_period, const void* l, size_t l_period, const void* u, size_t u_period,
                   const void* c, size_t c_period, void* out, void* dx, void* workspace, size_t workspace_bytes,
                   void* stream);
int rime_prior_bwd(int dtype, const void* dx, const void* g, size_t N, void* gx, void* stream);

/* ---------------------------------------------------------------------------------------
 * Correlated-noise likelihood: the quadratic form of the residual with an inverse covariance along ONE data axis
 * (optim.apply_icov, cov_axis 'bl' / 'time' / 'freq' / 'pix'; the reference's own branches cannot run, optim.py:1899-1913).
 * The data are viewed as (O, n, I) complex with the covariance axis in the middle; icov is (O*I, n, n) complex, batch
 * b = o*I + i, each matrix row-major and HERMITIAN (an inverse covariance; not checked: the backward relies on it).
 *     r = pred - data;  y[o,a,i] = sum_c icov[b][a][c] r[o,c,i];  q[b] = Re sum_a conj(r[o,a,i]) y[o,a,i];  out = sum_b q[b]
 *     backward: gpred[o,a,i] = 2 g y[o,a,i],  g T [1] (g_per_batch 0) or T [O*I] (g_per_batch 1)
 *   pred, data (NULL -> 0), y, gpred: T [O, n, I, 2], aligned to one complex number (8 bytes RIME_F32, 16 RIME_F64);
 *   icov T [O*I, n, n, 2], 16-byte aligned;  q T [O*I];  out T [1]
 *   y, q, out: each may be NULL (not wanted), not all three.  icov is read once; y makes the backward a scaling of y.
 * Deterministic: row terms and partial sums in double, added in a fixed order (workspace: rime_icov_workspace bytes).
 * rime_icov_plan: the launch plan of a shape without a device, plan_host[10] = {lanes per row, complex per load, tile T,
 *   row splits, rows per split, grid, LDS bytes of the staged residual, LDS bytes in all, the limit of the former, tile
 *   along o (I = 1)}.  RIME_EUNSUPPORTED: n too long for the LDS staging even at T = 1 (callers fall back to torch).
 * RIME_EINVAL: unknown dtype, O, n or I <= 0, a null pred / icov, no output, a misaligned pointer; RIME_EWORKSPACE after these.
 * ------------------------------------------------------------------------------------- */
int rime_icov_plan(int dtype, long long O, int n, long long I, int* plan_host);
size_t rime_icov_workspace(int dtype, long long O, int n, long long I);
int rime_icov_fwd(int dtype, const void* pred, const void* data, const void* icov, long long O, int n, long long I,
                  void* y, void* q, void* out, void* workspace, size_t workspace_bytes, void* stream);
int rime_icov_bwd(int dtype, const void* y, const void* g, int g_per_batch, long long O, int n, long long I,
                  void* gpred, void* stream);

/* ---------------------------------------------------------------------------------------
 * Full PSF matrix of the imaging path, P = D A^T w conj(A) with A = conj(fringe) beam (imaging.py:818-861), as a fused
 * phasor-Gram product: A is never built.
 *     S[f,i,j] = sum_b w[b,f] cos(2 pi nu_f/c (b_b.s_i - b_b.t_j));   out[f, rows[i], cols[j]] (= or +=) rs[f,i] cs[f,j] S[f,i,j]
 *   blvecs double [Nbl,3]; freqs double [Nf]; w T, element (b, f) at b w_sb + f w_sf (w_sf 0: one weight per baseline);
 *   sr double [3, ld_sr]: the Pr row directions s_i; sq double [3, ld_sq]: the Pq column directions t_j, or NULL: the
 *   rows again (symmetric form: only tile pairs ti <= tj are computed and stored twice, Pq and ld_sq are ignored);
 *   rs T [Nf, Pr], cs T [Nf, Pq], NULL -> 1;  rows int [Pr], cols int [Pq]: index maps into out, NULL -> identity; the
 *   caller guarantees unique, in-range entries;  out T [Nf, ldr, ldc];  accumulate 0: =, 1: +=.
 * The phase is formed in double, reduced to [-1/2, 1/2] turns and evaluated with one sincos of T per channel.  Every
 * output element is written by one work-group: no atomics, bit-identical from run to run.
 * RIME_EINVAL, before any HIP call: unknown dtype; a null blvecs / freqs / w / sr / out; Nbl, Nf, Pr (Pq with sq) <= 0;
 *   Nf > 65535; a negative w stride; ld_sr < Pr, ld_sq < Pq; ldr (ldc) <= 0 or, with the identity map, < Pr (Pq);
 *   accumulate not 0 / 1.
 * ------------------------------------------------------------------------------------- */
int rime_psf_gram(int dtype, const double* blvecs, const double* freqs, const void* w, long long w_sb, long long w_sf,
                  int Nbl, int Nf, const double* sr, long long ld_sr, int Pr, const double* sq, long long ld_sq, int Pq,
                  const void* rs, const void* cs, const int* rows, const int* cols, void* out, long long ldr,
                  long long ldc, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------
 * Gain application  V' = G1 V G2^dagger  per (baseline, time, channel) -- the post-RIME calibration
 * step, calibration._apply_cal (calibration.py:2412-2487; complex visibilities, no undo / covariance),
 * SURVEY section 8(f) item 3.  NP = 1 (1-pol) or 2; diag != 0 with NP = 2 is the reference's '2pol' mode
 * (diagonal products only, off-diagonal results zero: linalg.diag_matmul, linalg.py:116-149).
 *   vis, out, gout, gvis, d1, d2   T [NP][NP][Nbl][Nt][Nf][2]   contiguous, interleaved complex
 *   gains                          complex T, element (p, q, a, t, f) at complex offset
 *                                  (p*NP+q)*gst_p + a*gst_a + t*gst_t + f*gst_f  (0 strides broadcast)
 *   a1, a2                         int32 [Nbl]   antenna slots of each baseline (< Nant)
 * Backward (torch's conjugate-gradient convention): gvis = G1^dagger gout G2 and the PER-BASELINE gain
 * gradients d1 = gout (V G2^dagger)^dagger (belongs to antenna a1), d2 = gout^dagger (G1 V) (to a2); the
 * caller reduces d1 / d2 over the baselines of each antenna (and over broadcast axes).
 * ------------------------------------------------------------------------------------- */
int rime_apply_cal_fwd(int dtype, int NP, int diag, const void* vis, const void* gains, const int* a1,
                       const int* a2, int Nbl, int Nt, int Nf, int Nant, long long gst_p, long long gst_a,
                       long long gst_t, long long gst_f, void* out, void* stream);
int rime_apply_cal_bwd(int dtype, int NP, int diag, const void* vis, const void* gains, const void* gout,
                       const int* a1, const int* a2, int Nbl, int Nt, int Nf, int Nant, long long gst_p,
                       long long gst_a, long long gst_t, long long gst_f, void* gvis, void* d1, void* d2,
                       void* stream);

/* ---------------------------------------------------------------------------------------
 * Redundant-visibility / per-baseline visibility model term (calibration.RedVisModel, VisModel: calibration.py:877-1209):
 *     out[p, b, t, f] = vis[p, b, t, f] + sign * model[p, red[b], tmap[t], f]        sign = +1 | -1 (undo)
 *   vis, out, gout   T [NP*NP][Nbl][Nt][Nf][2]   contiguous, interleaved complex; vis NULL: the inflated model alone
 *   model            complex T, element (p, r, t', f) at complex offset p*mst_p + r*mst_r + t'*mst_t + f*mst_f
 *                    (strides >= 0, 0 broadcasts), r < Nred, t' < Ntm
 *   red              int32 [Nbl] (device): group of every baseline;  tmap int32 [Nt] (device): model time of every time, or
 *                    NULL for the identity (then Ntm must be Nt)
 *   gmodel           T [NP*NP][Nred][Ntm][Nf][2]  contiguous
 * Forward: one pass, gather + time selection + add fused.  Backward:
 *     gmodel[p, r, t', f] = sign * sum_{t: tmap[t] = t'} sum_{b: red[b] = r} gout[p, b, t, f]
 * as a segmented reduction over two CSR tables (device, int32) that the caller builds on the host: goff [Nred + 1] / gmem [Nbl]
 * (the baselines of every group) and toff [Ntm + 1] / tmem [Nt] (the times of every model time).  Lanes run along
 * (model time, channel); the 4 waves of a block take the members w, w + 4, ... of a group in ascending list position and the
 * partial sums are added through LDS in wave order: the summation order is a function of the tables alone (bit-reproducible).
 * Every element of gmodel is written exactly once, 0 for a group or model time without members; no atomics, no workspace.
 * Checked before any HIP call (RIME_EINVAL): null pointers (vis and tmap may be null), NP outside {1, 2}, an extent <= 0, an
 * unknown dtype, sign outside {+1, -1}, a negative stride, tmap NULL with Ntm != Nt.  The tables live on the device: the
 * caller checks them where it builds them (entries in range, offsets non-decreasing, last offset Nbl / Nt); the kernels
 * never read outside gout / model for a table that breaks this, but the result is then undefined.
 * ------------------------------------------------------------------------------------- */
int rime_redvis_fwd(int dtype, int NP, const void* vis, const void* model, const int* red, const int* tmap,
                    int Nbl, int Nt, int Nf, int Nred, int Ntm, long long mst_p, long long mst_r,
                    long long mst_t, long long mst_f, int sign, void* out, void* stream);
int rime_redvis_bwd(int dtype, int NP, const void* gout, const int* goff, const int* gmem, const int* toff,
                    const int* tmem, int Nbl, int Nt, int Nf, int Nred, int Ntm, int sign, void* gmodel,
                    void* stream);

/* ---------------------------------------------------------------------------------------
 * L-BFGS search direction in its compact form (bfgs.LBFGS, bfgs.two_loop_recursion; reference bfgs.py:619-678): the
 * two-loop recursion over m pairs (s_j, y_j) with the starting matrix gamma * diag(d) restated as one pass of inner products,
 * an m x m recurrence on the host and one linear combination.
 *   s_rows, y_rows   DEVICE arrays of m device addresses, oldest pair first; each address is a contiguous T [N], aligned to
 *                    sizeof(T) (a row that is not 16-byte aligned is read with element loads; the result has the same bits)
 *   v T [N];  d T [N] real diagonal or NULL (ones);  complex vectors are passed as their interleaved real views of length 2 N
 * rime_lbfgs_dots: out is double [2][m], out[0][j] = s_j . v, out[1][j] = y_j . (d o v); with 0 <= k < m (the index of a new
 *   pair that is already in the tables; k = -1: none) out is double [5][m] with also out[2][j] = s_j . y_k, out[3][j] = y_j . s_k,
 *   out[4][j] = y_j . (d o y_k).  Products and the per-lane chains (64 bytes of a row) run in T, every sum across lanes, waves
 *   and work-groups in float64; work-groups write partial sums to the workspace (rime_lbfgs_workspace(m, N) bytes, either
 *   dtype) and a second kernel of the same call adds them in a fixed order: no atomics, bit-reproducible, and a row's results
 *   do not depend on k, m or the other rows.
 * rime_lbfgs_combine: r T [N] = gamma * d o (v - sum_j a_j y_j) + sum_j b_j s_j in one pass; a, b double [m] on the device.
 * Checked before any HIP call: RIME_EINVAL for m < 1, N < 1, an unknown dtype, a null table, v, out, a, b or r, k outside
 * [-1, m); RIME_EWORKSPACE for a null or short workspace.  The tables live on the device and are not inspected by the host.
 * ------------------------------------------------------------------------------------- */
size_t rime_lbfgs_workspace(int m, long long N);
int rime_lbfgs_dots(int dtype, const void* const* s_rows, const void* const* y_rows, int m, long long N, const void* v,
                    const void* d, int k, double* out, void* workspace, size_t workspace_bytes, void* stream);
int rime_lbfgs_combine(int dtype, const void* const* s_rows, const void* const* y_rows, int m, long long N, const void* v,
                       const void* d, const double* a, const double* b, double gamma, void* r, void* stream);

/* ---------------------------------------------------------------------------------------
 * The two passes over the dense inverse Hessian of bfgs.BFGS (reference bfgs.py:169-235, where the update is the two matrix
 * products V^T H V + rho s s^T) and of the dense replay of the factored form (bfgs.FactoredInvHessian.to_dense).
 *   H   real T [N][ld], ld >= N; only columns 0 .. N - 1 of a row are read or written.  A base and an ld that are multiples of
 *       16 bytes are served with 16-byte accesses, any other placement with element accesses of the same elements: same bits.
 * rime_bfgs_matvec: r[i][c] = sum_j H[i][j] x[j][c], x and r T [N][nrhs], nrhs 1 or 2 (2: the interleaved real view of a complex
 *   vector against the real H).  Summation order, per row and right-hand side, all in T: with W = 16 / sizeof(T), lane l of the
 *   64 lanes of a wave runs one chain acc = fma(H[i][j], x[j], acc) from acc = 0 over its columns j in ascending order -- the
 *   columns 64 W q + W l ... + W - 1 for q = 0, 1, ... -- and the 64 chains are then added pairwise by a butterfly, partners 32, 16,
 *   8, 4, 2, 1 lanes apart.  A work-group owns whole rows; no atomics, no workspace: a row's bits depend on the row, x and N alone.
 * rime_bfgs_rank2: in place, per element and in T with every operation rounded on its own,
 *       H[i][j] = fma(T(b), x_i * x_j, fma(T(a), x_i * z_j + z_i * x_j, H[i][j]))
 *   (the two products of the sum are rounded, then added; x_i * x_j is rounded, then scaled).  The expression is symmetric under
 *   i <-> j, so a bit-symmetric H stays bit-symmetric.  BFGS update: x = s, z = H y, a = -rho, b = rho^2 (y . H y) + rho;
 *   the shell (I + u v^T) H (I + v u^T) of a symmetric H: x = u, z = H v, a = 1, b = v . H v.
 * x, z and r must not overlap the rows of H.  Checked before any HIP call: RIME_EINVAL for an unknown dtype, N < 1 (or above
 * 2^31 - 1), ld < N, a null pointer, nrhs outside {1, 2}, a non-finite a or b, or a vector that overlaps H.
 * ------------------------------------------------------------------------------------- */
int rime_bfgs_matvec(int dtype, const void* H, long long ld, long long N, const void* x, int nrhs, void* r, void* stream);
int rime_bfgs_rank2(int dtype, void* H, long long ld, long long N, const void* x, const void* z, double a, double b,
                    void* stream);

/* ---------------------------------------------------------------------------------------
 * One leapfrog stage of Hamiltonian Monte Carlo with a diagonal mass (sampler.leapfrog, sampler.HMC.K; reference
 * sampler.py:391-450, 1433-1583): momentum kick, position drift and kinetic energy in one pass over the flat parameter vector.
 *   q, p   T [N] updated in place;  g T [N] the potential's gradient;  eps T [N] step size per element or NULL (ones);
 *   c      T [N] diagonal Cholesky factor of the covariance or NULL (ones);  all aligned to sizeof(T) (a base that is not
 *          16-byte aligned takes element accesses; the result has the same bits);  complex parameters are passed as their
 *          interleaved real views of length 2 N with eps and c repeated per component
 * Per element, in T, in this order:
 *     kick  != 0:   p <- fma(-(T(kick) * eps), g, p)
 *     drift != 0:   q <- fma(T(drift) * eps, c * (c * p), q)          with the updated p
 *     energy:       energy[0] = 1/2 sum (c * p)^2  (double, device)   with the updated p
 *   kick = drift = 0 with energy set is the energy-only pass.  g may be NULL only for kick = 0, q only for drift = 0.
 *   The sum runs as the per-lane chains (64 bytes of p) in T, then float64 across lanes, waves and work-groups; work-groups
 *   write partial sums to the workspace (rime_hmc_workspace(N) bytes, either dtype; needed only with energy) and a second
 *   kernel of the same call adds them in a fixed order: no atomics, bit-reproducible, and the same bits with and without
 *   the kick of the same call.
 * Checked before any HIP call: RIME_EINVAL for an unknown dtype, N < 0, a null p, a null g with kick != 0, a null q with
 * drift != 0, a NaN flag or a non-zero flag that rounds to zero in T; RIME_EWORKSPACE for a null or short workspace with energy.
 * ------------------------------------------------------------------------------------- */
size_t rime_hmc_workspace(long long N);
int rime_hmc_step(int dtype, long long N, void* q, void* p, const void* g, const void* eps, const void* c, double kick,
                  double drift, double* energy, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * One step of a recycled HMC trajectory (recycled.RecycledHMC; reference sampler.py:799-893), which keeps every intermediate
 * state: the closing half kick of step i with its kinetic energy, the snapshot of the state, and the opening half kick and
 * drift of step i + 1 in one pass.  Vectors, eps and c as in rime_hmc_step; q_out, p_out T [N] (row i of the trajectory).
 * Per element, in T, in this order:
 *     p1 = fma(-(T(half) * eps), g, p);      energy[0] = 1/2 sum (c * p1)^2;      q_out = q;   p_out = p1
 *     drift != 0:   p2 = fma(-(T(half) * eps), g, p1);   p <- p2;   q <- fma(T(drift) * eps, c * (c * p2), q)
 *     drift == 0:   p <- p1
 *   The energy is summed in the order of rime_hmc_step's, through the workspace of rime_hmc_workspace(N) bytes.
 * Bit contract: q, p, q_out, p_out and energy carry the bits of rime_hmc_step(kick = half, drift = 0, energy), a copy of q and
 *   p to q_out and p_out, and rime_hmc_step(kick = half, drift) when drift != 0 -- two half kicks, never one full kick -- for
 *   every N, dtype, alignment and null combination.
 * Checked before any HIP call: RIME_EINVAL for an unknown dtype, N < 0, a null q, p, g, q_out, p_out or energy, a NaN flag,
 * half = 0, q_out or p_out overlapping q, p, g, eps, c or each other, a non-zero flag that rounds to zero in T; RIME_EWORKSPACE for a
 * null or short workspace (looked at before the rounding, as in rime_hmc_step).
 * ------------------------------------------------------------------------------------- */
int rime_hmc_recycle(int dtype, long long N, void* q, void* p, const void* g, const void* eps, const void* c, double half,
                     double drift, void* q_out, void* p_out, double* energy, void* workspace, size_t workspace_bytes,
                     void* stream);

/* ---------------------------------------------------------------------------------------
 * One leaf of the No-U-Turn sampler's tree (nuts.NUTS.build_tree; reference sampler.py:1104-1140 with the criterion of
 * sampler.py:1402-1430): a leapfrog step of the signed size h from an edge state of the tree, which stays as it is, in two
 * launches around the evaluation of the potential's gradient at the new position.
 *   all vectors T [N], flat and real as in rime_hmc_step (complex parameters as their interleaved real views);  eps, c as there,
 *   each NULL for ones;  h the signed step: direction x step size for a scalar step size, +-1 with eps a vector
 * rime_nuts_leaf_open, out of place (q0, p0, g0 the edge state and its gradient, read only; q1, p1 written), per element, in T:
 *     p1 = fma(-(T(h/2) * eps), g0, p0);      q1 = fma(T(h) * eps, c * (c * p1), q0)
 *   the bits of a copy of q0, p0 followed by rime_hmc_step(kick = h/2, drift = h).
 * rime_nuts_leaf_close, in place on p1 (g1 the gradient at q1), per element, in T:
 *     p1 <- fma(-(T(h/2) * eps), g1, p1)
 *   and, with the updated p1, three doubles on the device:
 *     out[0] = 1/2 sum (c * p1)^2;    out[1] = sum (q1 - q_far) * p_far;    out[2] = sum (q1 - q_far) * p1
 *   (q_far, p_far: the state at the far edge of the tree the leaf is tested against; the no-U-turn criterion of Hoffman & Gelman
 *   is the sign of these two sums, negated for h < 0).  q_far = p_far = NULL skips the two projections: out[1], out[2] are not
 *   written.  The difference q1 - q_far is rounded once in T; each sum runs as the per-lane chains (64 bytes of a vector) of fused
 *   multiply-adds in T, then float64 across lanes, waves and work-groups in the order of rime_hmc_step's energy: work-groups
 *   write partial sums to the workspace (rime_nuts_workspace(N) bytes, either dtype) and a second kernel of the same call adds
 *   them.  No atomics, bit-reproducible, and out[0] carries the bits of rime_hmc_step's energy for the same p1, g1, eps, c.
 * Checked before any HIP call: RIME_EINVAL for an unknown dtype, N < 0, a null q0, p0, g0, q1, p1, g1 or out, only one of q_far
 * and p_far, q1 or p1 of open overlapping one of its inputs or each other, a NaN h, h = 0 or an h whose half rounds to zero in T;
 * RIME_EWORKSPACE for a null or short workspace (looked at before the rounding of h, as in rime_hmc_step).
 * ------------------------------------------------------------------------------------- */
size_t rime_nuts_workspace(long long N);
int rime_nuts_leaf_open(int dtype, long long N, const void* q0, const void* p0, const void* g0, void* q1, void* p1,
                        const void* eps, const void* c, double h, void* stream);
int rime_nuts_leaf_close(int dtype, long long N, const void* q1, void* p1, const void* g1, const void* eps, const void* c,
                         double h, const void* q_far, const void* p_far, double* out, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * One leapfrog stage with a block-dense mass matrix (massmat.leapfrog, massmat.HMC, massmat.NUTS; reference sampler.py:260-450,
 * 489-546, 1516-1554): the flat real vector of rime_hmc_step, with a DEVICE table of nblocks blocks of 64 bytes each:
 *     struct rime_mass_block { const void* L; long long ld, off; int n, nrhs; long long reserved[4]; };
 *   L      real T [n][ld], ld >= n: the lower-triangular Cholesky factor of one key's covariance; only L[i][j], j <= i, is read.
 *          A base and an ld that are multiples of 16 bytes take 16-byte loads (of groups wholly at or below the diagonal), any
 *          other placement element loads of the same elements: same bits.
 *   off    first flat element of the block, which covers off ... off + n nrhs - 1;  nrhs 1 (a real key) or 2 (the interleaved
 *          real view of a complex key: the same real L acts on both components).  Blocks do not overlap.  Elements that no
 *          block covers are diagonal with the factor c (NULL: ones), as in rime_hmc_step.
 * rime_mass_project, per element and in T:
 *     p_out = fma(-(T(kick) * eps), g, p_in)        (kick = 0: p_in is used as it is; g and p_out may be NULL)
 *     z = L^T p_out on every block,  z = c * p_out elsewhere
 *   With kick != 0, p_out must not overlap p_in; z must overlap neither.
 * rime_mass_drift, per element and in T:
 *     q_out = fma(T(drift) * eps, L z, q_in) on every block,  fma(T(drift) * eps, c * z, q_in) elsewhere     (drift != 0)
 *   q_out may be q_in; with drift = 0 nothing is written and q_in, q_out may be NULL.  out, double [3] on the device or NULL:
 *     out[0] = 1/2 sum z^2;   out[1] = sum (q - q_far) * p_far;   out[2] = sum (q - q_far) * p
 *   with q the position after the call (q_out, or q_in when q_out is NULL); out[1], out[2] only when p, q_far and p_far are
 *   given (all three or none).  The three sums run in the order of rime_hmc_step's energy / rime_nuts_leaf_close over ALL
 *   elements; partial sums go to the workspace (rime_mass_workspace(N) bytes, either dtype; needed only with out).
 * Summation order of the triangular products, all in T, W = 16 / sizeof(T):
 *   L z     row i: lane l of a wave runs one chain acc = fma(L[i][j], z[j], acc) from 0 over its columns j <= i ascending -- the
 *           columns 256 W q + (64 g + l) W + e, q = 0, 1, ..., g = 0 .. 3, e < W -- then the butterfly over the 64 lanes
 *           (partners 32, 16, 8, 4, 2, 1 apart).
 *   L^T p   column j: slot s of 32 runs one chain acc = fma(L[i][j], p[i], acc) from 0 over the rows i >= j, i = s (mod 32),
 *           ascending; slots 8 w + u are added by a butterfly over u (partners 4, 2, 1), then ((w0 + w1) + w2) + w3 over w.
 *   An output element's bits depend on its own block's L, n and the vector alone: not on ld, the alignment, the other blocks or
 *   the launch.  No atomics; each call is a fixed sequence of kernels on `stream`, and no work-group waits for another.  With
 *   nblocks = 0, project then drift give the bits of rime_hmc_step (p, q, energy) and of rime_nuts_leaf_close (the three sums).
 * Checked before any HIP call: RIME_EINVAL for an unknown dtype, N < 0, nblocks < 0, a null table with nblocks > 0, a null p_in
 * or z, a null g or p_out with kick != 0, a null q_in or q_out with drift != 0, the overlaps named above, only some of p, q_far,
 * p_far, a NaN kick or drift or one that rounds to zero in T; RIME_EWORKSPACE for a null or short workspace with out (looked at
 * before the rounding, as in rime_hmc_step).  The device table is not inspected by the host; an entry that does not fit the
 * vector (n < 1, nrhs outside {1, 2}, ld < n, off < 0, off + n nrhs > N) is skipped on the device.
 * ------------------------------------------------------------------------------------- */
size_t rime_mass_workspace(long long N);
int rime_mass_project(int dtype, long long N, const void* blocks, int nblocks, const void* p_in, const void* g, const void* eps,
                      const void* c, double kick, void* p_out, void* z, void* stream);
int rime_mass_drift(int dtype, long long N, const void* blocks, int nblocks, const void* z, const void* q_in, const void* eps,
                    const void* c, double drift, void* q_out, const void* p, const void* q_far, const void* p_far, double* out,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Grouped block mat-vec of a flattened operator tree (hmat.BaseMat.mat_vec_mul / mat_mat_mul; reference hmat.py): y (+)=
 * scalar * A x, A given as a DEVICE table of ntiles tiles of 64 bytes each:
 *     struct rime_hmat_tile { const void* a; long long ld, src_off, dst_off; double scale; int rows, cols, flags, stage;
 *                             long long reserved; };
 *   a         real matrix T [rows][ld] (ld >= cols) as stored, or, with RIME_HMAT_DIAG, a vector T [rows] (cols = 1) or ONE
 *             value repeated rows times (cols = 0); aligned to sizeof(T) only: a base or ld that is not a multiple of 16 bytes
 *             takes element loads of the same elements (the result has the same bits), any other 16-byte loads
 *   flags     RIME_HMAT_TRANS 1: the tile applies the transpose of the stored matrix (cols outputs from rows inputs);
 *             RIME_HMAT_DIAG 2;  RIME_HMAT_SRC_SCRATCH 4: the input segment lies in the scratch vector, not in x
 *   src_off, dst_off   first element of the input / output segment in its vector;  stage: the launch the tile belongs to
 * The destination of a tile is fixed by the row ranges that list it.  ranges: DEVICE long long [5] per work-group, those of
 * stage s at entries stage_first[s] ... stage_first[s + 1] - 1 (stage_first: HOST int [nstages + 1]): {flags, first row, rows
 * (at most 256), first entry of tile_ids, entries}; flags 1: the rows are rows of the scratch vector (written as the plain sum),
 * 2: the rows of y are added to whatever `accumulate` says (the later stages).  tile_ids: DEVICE int, the tiles of each range
 * in the order they are visited.  Stage 0 must cover every row of y once (a row without tiles receives 0); the ranges of one
 * stage must not overlap.  x, y, scratch: T [n][nrhs], the nrhs right-hand sides interleaved per element (a complex vector is
 * its interleaved real view with nrhs = 2); any nrhs >= 1, served four columns per launch.  The scratch vector is the
 * workspace: rime_hmat_workspace(dtype, scratch_rows, nrhs) bytes.
 * Arithmetic, all in T, per output row and right-hand side: acc = 0; for each tile of the range that touches the row, in
 * tile_ids order, acc = fma(T(scale), s, acc) with s the tile's sum (W = 16 / sizeof(T)):
 *   plain form, cols > 32 W    lane l of a wave holds columns 128 W c + (64 g + l) W + e (chunk c ascending, g = 0, 1, e < W)
 *                 and runs one chain p = fma(A[i][col], x[col], p) over them in ascending order; s is the butterfly sum of
 *                 the 64 chains (p += p of lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1)
 *   plain form, cols <= 32 W   G = the power of two >= cols / W lanes share the row, lane g its columns g W + e as one chain;
 *                 s is the butterfly sum over the G lanes (^ G / 2, ..., ^ 1)
 *   TRANS, cols > 32 W         wave w of the four runs one chain over the stored rows j = w, w + 4, ... ascending;
 *                 s = ((p0 + p1) + p2) + p3
 *   TRANS, cols <= 32 W        with G as above and S = 64 / G, wave w and slot u < S run one chain over the stored rows
 *                 j = S w + u, + 4 S, ... ascending; s is the sum of the 4 S chains in the order (w, u), w major, from the left
 *   DIAG          s = a[i] * x[i]
 * then y = T(scalar) * acc, or fma(T(scalar), acc, y) when accumulating; scratch = acc.  No atomics and no communication
 * between work-groups: bit-reproducible, and a row's result depends on its own tiles and their order only.  Stages are
 * separate launches on `stream`.
 * Checked before any HIP call: RIME_EINVAL for an unknown dtype, ntiles < 0, nstages outside [1, 8], nrhs < 1, scratch_rows
 * < 0, a decreasing or negative stage_first, a null ranges, stage_first, x or y, a null tiles or tile_ids with ntiles > 0;
 * then RIME_EWORKSPACE for a null or short workspace with scratch_rows > 0.  The device tables are not inspected by the host.
 * ------------------------------------------------------------------------------------- */
#define RIME_HMAT_TRANS 1
#define RIME_HMAT_DIAG 2
#define RIME_HMAT_SRC_SCRATCH 4
size_t rime_hmat_workspace(int dtype, long long scratch_rows, int nrhs);
int rime_hmat_apply(int dtype, const void* tiles, int ntiles, const long long* ranges, const int* tile_ids,
                    const int* stage_first, int nstages, long long scratch_rows, const void* x, void* y, int nrhs,
                    double scalar, int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * LST alignment of drift-scan visibilities (telescope_model.vis_rephase, VisData.lst_rephase / time_nn_interp /
 * time_average; reference dataset.py:1363-1566, telescope_model.py:594-645): rephasing, weighting and the average of the
 * integrations of every bin in one pass (csrc/lstbin.hip).  Tensors [Npp, Nbl, Nt, Nf] in, [Npp, Nbl, Nbin, Nf] out,
 * channel fastest, contiguous, aligned to their element size only (a base off 16 bytes, or an Nf that is not a multiple of
 * 16 / sizeof(T) channels, takes element accesses of the same elements: same bits); data / avg complex (interleaved T),
 * wgts / cov / sum_w / avg_cov real T, flags / avg_flag one byte per element (0: unflagged).
 * Bins: a CSR table bin_ptr [Nbin + 1], members [Nmem] (time indices of every bin, ascending table position is the order
 * of summation); a time may be in no bin (dropped) or in several.  For every (p, b, bin k, f), over the table positions m
 * of the bin with t = members[m]:
 *     sum_w    = sum w[p, b, t, f]                                                   (w = 1 when wgts is null)
 *     avg      = sum w V[p, b, t, f] exp(2 pi i freqs[f] tau[b, j]) / max(sum_w, 1e-40)
 *     avg_cov  = sum w^2 cov[p, b, t, f] / max(sum_w, 1e-40)^2                       (cov and avg_cov both given or both null)
 *     avg_flag = 1 where every member is flagged (an empty bin: 1)                   (flags and avg_flag both or neither)
 * tau: DEVICE float64 [Nbl, Nt] with j = t, or, with tau_by_member = 1, [Nbl, Nmem] with j = m (one delay per table
 * position: a time that serves several bins); null: no phasor is generated.  freqs: DEVICE float64 [Nf] (needed with tau).
 * The product freqs[f] * tau is formed and reduced to [-1/2, 1/2] turns in float64, sine and cosine are taken in T.  data
 * null: V = 1, i.e. with singleton bins and no weights avg is the phasor itself.  sum_w may be null (not written).
 * rime_vis_timeavg_bwd: the gradient with respect to the data ONLY (weights, tau and cov receive none),
 *     gdata[p, b, t, f] = sum over the table positions m holding t of
 *                         w[p, b, t, f] conj(phasor) gavg[p, b, pos_bin[m], f] / max(sum_w[p, b, pos_bin[m], f], 1e-40)
 * through the transposed table t_ptr [Nt + 1], t_pos [Nmem] (table positions of every time, ascending) and pos_bin [Nmem]
 * (the bin of every table position); every element of gdata is written (0 for a time in no bin).  sum_w: as the forward wrote.
 * No atomics, one summation chain per output element in table order: bit-reproducible.
 * The *_host arguments are HOST copies of the tables; the kernels read the DEVICE ones.  Checked before any HIP call, on the
 * host copies: RIME_EINVAL for an unknown dtype, a negative size, tau_by_member outside {0, 1}, a null avg / gavg / sum_w (bwd) /
 * gdata / table, tau without freqs, cov or flags without their output (or the reverse), a table that does not start at 0,
 * decreases or does not end at Nmem, a member outside [0, Nt), a t_pos outside [0, Nmem), a pos_bin outside [0, Nbin).  The
 * device tables are not inspected by the host (the kernels skip entries that point outside).
 * ------------------------------------------------------------------------------------- */
int rime_vis_timeavg_fwd(int dtype, const void* data, const void* wgts, const void* cov, const void* flags, const double* tau,
                         int tau_by_member, const double* freqs, const int* bin_ptr, const int* members,
                         const int* bin_ptr_host, const int* members_host, int Npp, int Nbl, int Nt, int Nf, int Nbin, int Nmem,
                         void* avg, void* sum_w, void* avg_cov, void* avg_flag, void* stream);
int rime_vis_timeavg_bwd(int dtype, const void* gavg, const void* wgts, const void* sum_w, const double* tau,
                         int tau_by_member, const double* freqs, const int* t_ptr, const int* t_pos, const int* pos_bin,
                         const int* t_ptr_host, const int* t_pos_host, const int* pos_bin_host, int Npp, int Nbl, int Nt,
                         int Nf, int Nbin, int Nmem, void* gdata, void* stream);

/* ---------------------------------------------------------------------------------------
 * Antenna mutual coupling of visibilities (calibration.VisCoupling; reference calibration.py:1258-1586), single polarisation:
 *     W = E V E^H (prod = BOTH),  E V (LEFT),  V E^H (RIGHT)         E = [I] + X o D   per (t, f), N x N complex
 * on one batched complex product kernel (csrc/coupling.hip) whose operands are read, and whose results are written, in place:
 *   x        complex T [N][N][Tm][Fm], Tm in {1, Nt}, Fm in {1, Nf} (1 broadcasts);  dly complex T [N][N][Nf] or NULL (ones)
 *   data     complex T [Nbl][Nt][Nf];  out, gout complex T [Nout][Nt][Nf];  gdata as data;  gx as x
 *   tab      int32 [N][N] (device): V[a][b] = data[row] for the word `row`, conj(data[row]) for `row | 1 << 30`, 0 for -1
 *   otab     int32 [N][N] (device): W[a][b] is output row `row`, -1: not an output.  Every output row names one entry.
 *   ftab     int32 [N][N] (device), backward: entry (a, b) holds the data row read unconjugated there, with 1 << 30 set when no
 *            entry reads that row conjugated (an auto-correlation), -1 elsewhere; needed with gdata
 * No (N^2, Nt, Nf) copy of the data is made and E is never materialised; the intermediate of a two-sided product lives in the
 * caller's workspace: rime_coupling_workspace(dtype, N, Nt, Nf, Tm, Fm, prod, stage) bytes, stage RIME_COUPLING_FWD (T = E V
 * for BOTH, else 0), RIME_COUPLING_BWD (T and P = G E for BOTH, plus one matrix when Tm != Nt or Fm != Nf) or
 * RIME_COUPLING_EXPAND_BWD (one matrix when Tm != Nt or Fm != Nf); 0 for arguments the calls below reject.
 * rime_coupling_bwd, with G the matrix that holds gout at the output entries and 0 elsewhere:
 *     gV = E^H G E,  gdata[row(a, b)] = gV[a][b] + conj(gV[b][a]) (the first term alone when the word carries 1 << 30),
 *     gE = G E V^H + G^H E V (LEFT: G V^H;  RIGHT: G^H V),  gx = gE o conj(dly), summed over t when Tm = 1 and over f when Fm = 1.
 *   gdata or gx may be NULL (not computed).  Rows of gdata that ftab does not name are not written.
 * rime_coupling_expand: the double-path matrix e [N][N][Nt][Nf] = [I] + Xd + Xd Xd, Xd = X o D, as a dense tensor to be passed
 *   as x (with dly NULL, addI 0) to the calls above;  rime_coupling_expand_bwd: gx = (ge + ge Xd^H + Xd^H ge) o conj(dly),
 *   summed over the broadcast axes.
 * Every output element is summed over k in ascending order by one thread (two products of a sum one after the other), the
 * broadcast sums t outer, f inner, ascending: no atomics, bit-reproducible.  float32 accumulates in float32, float64 in float64.
 * Checked before any HIP call: RIME_EINVAL for a null pointer (dly may be null; gdata or gx, not both), an unknown dtype, prod
 * or stage, N, Nt, Nf, Nbl or Nout < 1, Tm outside {1, Nt}, Fm outside {1, Nf}, addI outside {0, 1}; RIME_EWORKSPACE for a null
 * or short workspace where one is needed.  The tables live on the device and are checked by the caller where they are built;
 * the kernel treats a row outside [0, Nbl) / [0, Nout) as -1 and never reads or writes outside the tensors.
 * ------------------------------------------------------------------------------------- */
#define RIME_COUPLING_BOTH 0
#define RIME_COUPLING_LEFT 1
#define RIME_COUPLING_RIGHT 2
#define RIME_COUPLING_FWD 0
#define RIME_COUPLING_BWD 1
#define RIME_COUPLING_EXPAND_BWD 2
size_t rime_coupling_workspace(int dtype, int N, int Nt, int Nf, int Tm, int Fm, int prod, int stage);
int rime_coupling_fwd(int dtype, const void* x, const void* dly, const void* data, const int* tab, const int* otab,
                      int N, int Nbl, int Nout, int Nt, int Nf, int Tm, int Fm, int addI, int prod, void* out,
                      void* workspace, size_t workspace_bytes, void* stream);
int rime_coupling_bwd(int dtype, const void* x, const void* dly, const void* data, const void* gout, const int* tab,
                      const int* otab, const int* ftab, int N, int Nbl, int Nout, int Nt, int Nf, int Tm, int Fm,
                      int addI, int prod, void* gdata, void* gx, void* workspace, size_t workspace_bytes, void* stream);
int rime_coupling_expand(int dtype, const void* x, const void* dly, int N, int Nt, int Nf, int Tm, int Fm, int addI,
                         void* e, void* stream);
int rime_coupling_expand_bwd(int dtype, const void* x, const void* dly, const void* ge, int N, int Nt, int Nf, int Tm,
                             int Fm, void* gx, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Mutual coupling of redundant visibilities (calibration.RedVisCoupling; reference calibration.py:1588-2115), single
 * polarisation:  Vc = A(eps) Vr + B(eps) conj(Vr)  without the two dense (Nout, Nin, Nt, Nf) matrices (csrc/redcoupling.hip).
 * What the forward adds up is one list of entries, int32 ent [Nent][4] (device) = (i, j | flag << 30, a, b), sorted by i:
 *     out[i][t][f] = sum over the entries of row i, ascending, of  coef (flag ? conj(data[j][t][f]) : data[j][t][f])
 *     coef = (a >= 0 ? C[a] : 1) (b >= 0 ? conj(C[b]) : 1),   C[c][t][f] = x[c][tm][fm] dly[c][f]
 *   x      complex T [Nterms][Tm][Fm], Tm in {1, Nt}, Fm in {1, Nf} (1 broadcasts);  dly complex T [Nterms][Nf] or NULL (ones)
 *   data   complex T [Nin][Nt][Nf];  out, gout complex T [Nout][Nt][Nf];  gdata as data;  gx as x
 *   roff   int32 [Nout + 1]: the entries of every row (ent is in row order)
 *   coff   int32 [Nin + 1], cmem int32 [Nent]: the entries that read every column, ascending
 *   toff   int32 [Nterms + 1], tmem int32 [Nmem]: per term the words `entry` (the term is a of the entry) and
 *          `entry | 1 << 30` (it is b), ascending in (entry, role); an entry with a == b is listed under both
 *   segterm, segstart int32 [Nseg], tsoff int32 [Nterms + 1]: every term's list cut into segments of `seg` words: the term and
 *          the first position in tmem of every segment, and the segments of every term
 * rime_redcoupling_bwd_data:      gdata[j] = sum over the readers of j of  conj(coef) gout[i]  (flag 0),  coef conj(gout[i])  (1);
 *   every element of gdata is written.
 * rime_redcoupling_bwd_coupling:  gx[c] = conj(dly[c]) sum over the words of term c of  conj(w) gout[i],  w = conj(C[b]) v  (role a)
 *   or  w' conj(gout[i]),  w' = C[a] v  (role b), v the visibility as the entry reads it; summed over t when Tm = 1 and over f
 *   when Fm = 1.  One wave adds the words of a segment in ascending order into the workspace (rime_redcoupling_workspace bytes:
 *   Nseg Nt Nf complex), then per (term, tm, fm) wave w of a block adds the segments w, w + 4, ... in ascending order (t outer
 *   of f), the lanes by a butterfly when Fm = 1, and wave 0 the four wave sums.  Terms without a word get zeros.
 * No atomics; every sum has an order fixed by the tables: bit-reproducible.  float32 accumulates in float32, float64 in float64.
 * Checked before any launch: RIME_EINVAL for a null pointer (dly may be null; tmem, segterm, segstart when Nmem = Nseg = 0), an
 * unknown dtype, Nout, Nin, Nterms, Nent, Nt or Nf < 1, Nout, Nin or Nent >= 2^30, Tm outside {1, Nt}, Fm outside {1, Nf}, Nmem or
 * Nseg < 0, Nseg > Nmem, one of Nmem and Nseg zero alone, seg outside [1, 2^20]; RIME_EWORKSPACE for a null or short workspace
 * where one is needed.  The tables live on the device and are checked by the caller where they are built; the kernels skip every
 * word that points outside and never read or write outside the tensors.
 * ------------------------------------------------------------------------------------- */
size_t rime_redcoupling_workspace(int dtype, int Nseg, int Nt, int Nf);
int rime_redcoupling_fwd(int dtype, const void* x, const void* dly, const void* data, const int* ent, const int* roff,
                         int Nout, int Nin, int Nterms, int Nent, int Nt, int Nf, int Tm, int Fm, void* out, void* stream);
int rime_redcoupling_bwd_data(int dtype, const void* x, const void* dly, const void* gout, const int* ent, const int* coff,
                              const int* cmem, int Nout, int Nin, int Nterms, int Nent, int Nt, int Nf, int Tm, int Fm,
                              void* gdata, void* stream);
int rime_redcoupling_bwd_coupling(int dtype, const void* x, const void* dly, const void* data, const void* gout, const int* ent,
                                  const int* toff, const int* tmem, const int* segterm, const int* segstart, const int* tsoff,
                                  int Nout, int Nin, int Nterms, int Nent, int Nmem, int Nseg, int seg, int Nt, int Nf, int Tm,
                                  int Fm, void* gx, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Sparse learnable mixing of a partly redundant array (calibration.PartialRedVisInflate; reference calibration.py:2178-2344;
 * csrc/partred.hip):
 *     out[p, i, t, f] = sum over the entries e of row i, e = roff[i] ... roff[i + 1] - 1 in that order, of c[e] V[p, col[e], t, f]
 *   V                complex T, element (p, j, t, f) at complex offset p*vst_p + j*vst_b + t*vst_t + f*vst_f (strides >= 0,
 *                    0 broadcasts), p < NP*NP, j < Nin
 *   c, gc            T [Nnz]  real: one coefficient per entry, and its gradient
 *   out, G           T [NP*NP][Nout][Nt][Nf][2]  contiguous, interleaved complex;  gV  T [NP*NP][Nin][Nt][Nf][2]  contiguous
 *   roff             int32 [Nout + 1] (device): the entries of every row are consecutive, in the caller's order
 *   col, row         int32 [Nnz] (device): column and row of every entry
 *   coff, cmem       int32 [Nin + 1], [Nnz] (device): the entries of every column, ascending entry number
 * rime_partred_fwd: one pass, one FMA per real component and term, lanes along (i, t, f); a row without entries gets 0.
 * rime_partred_bwd_data:   gV[p, j, t, f] = sum over the entries e of column j, ascending, of c[e] G[p, row[e], t, f]: a block
 *   owns 64 (time, channel) columns of one (p, j), its 4 waves take the members w, w + 4, ... in ascending position and wave 0
 *   adds the partial sums from LDS in wave order; a column without entries gets 0.
 * rime_partred_bwd_coeff:  gc[e] = sum over (p, t, f) of Re V Re G + Im V Im G with V = V[p, col[e], t, f], G = G[p, row[e], t, f]:
 *   one block of 256 threads per row, 4 entries per sweep of the row of G; thread k adds the elements k, k + 256, ... in T (the
 *   real product first, the imaginary one fused onto it), then in float64 the butterfly across the wave (partners 32 ... 1) and
 *   the 4 waves in order, rounded to T once.
 * No atomics, no workspace, no prior memset; every element of out, gV and gc is written exactly once and every summation order
 * is a function of the tables alone (bit-reproducible).  Checked before any launch (RIME_EINVAL): an unknown dtype, a null
 * pointer, NP outside {1, 2}, Nout, Nin, Nnz, Nt or Nf < 1, a negative stride.  The tables live on the device and are checked by
 * the caller where they are built (entries in range, offsets non-decreasing from 0 to Nnz, every entry once per list); the
 * kernels clamp every table read and never read or write outside the tensors, but for such a table the result is undefined.
 * ------------------------------------------------------------------------------------- */
int rime_partred_fwd(int dtype, int NP, const void* V, const void* c, const int* roff, const int* col,
                     int Nout, int Nin, int Nnz, int Nt, int Nf, long long vst_p, long long vst_b,
                     long long vst_t, long long vst_f, void* out, void* stream);
int rime_partred_bwd_data(int dtype, int NP, const void* G, const void* c, const int* row, const int* coff,
                          const int* cmem, int Nout, int Nin, int Nnz, int Nt, int Nf, void* gV, void* stream);
int rime_partred_bwd_coeff(int dtype, int NP, const void* V, const void* G, const int* roff, const int* col,
                           int Nout, int Nin, int Nnz, int Nt, int Nf, long long vst_p, long long vst_b,
                           long long vst_t, long long vst_f, void* gc, void* stream);

/* ---------------------------------------------------------------------------------------
 * Lightcone sampling of periodic simulation boxes (cosmology.cube2lcone / cube2map; reference cosmology.py:237-427;
 * csrc/lcone.hip): every (radius i, pixel p) output in one launch,
 *     out[i, p] = sum over s < S of  weight[i, s] sample(sims[cube_idx[i, s]], position(i, p))
 *   sims      T [Nsim][Nx][Ny][Nz], contiguous (z fastest);  out  T [Nr][Npix]
 *   mode      RIME_LCONE_SPHERE: position = (vec[:, p] * dc[i]) / sim_res per axis, vec DEVICE float64 [3][Npix];
 *             RIME_LCONE_PLANE: pixel p = x Ny + y is the cube's own column (x, y), only z = dc[i] / sim_res is sampled;
 *             Npix must be Nx Ny and vec is not read (may be null)
 *   interp    RIME_LCONE_NEAREST: the voxel at rint(position) (half to even);  RIME_LCONE_LINEAR: trilinear (PLANE: linear
 *             in z) between floor(position) and floor(position) + 1, fraction position - floor(position) rounded once to T
 *   dc        DEVICE float64 [Nr];  cube_idx DEVICE int32 [Nr][3], weight DEVICE float64 [Nr][3]: the radial stencil of
 *             every radius, its first S (1 ... 3) columns used, weights rounded once to T;  cube_idx_host: a HOST copy
 *   rx ry rz  the roll of the cube along its axes, reduced to [0, N): the rolled cube at i is the cube at (i - r) mod N
 * Positions are float64 for either T; indices are taken modulo the extents, non-negative, the box tiling all space; offsets
 * are 64-bit.  One lane per output, a fixed operation order (csrc/lcone.hip), no atomics: bit-reproducible.
 * Checked before any HIP call (RIME_EINVAL): an unknown dtype, mode or interp, S outside [1, 3], an extent, Nr or Npix < 1, a
 * null sims, dc, cube_idx, weight, cube_idx_host or out, a null vec in SPHERE mode, Npix != Nx Ny in PLANE mode, sim_res not
 * positive and finite, a roll outside [0, N), a cube_idx_host entry (of the first S columns) outside [0, Nsim).  The device
 * table is not inspected by the host (the kernel clamps its entries).
 * ------------------------------------------------------------------------------------- */
#define RIME_LCONE_SPHERE 0
#define RIME_LCONE_PLANE 1
#define RIME_LCONE_NEAREST 0
#define RIME_LCONE_LINEAR 1
int rime_lcone_fwd(int dtype, int mode, int interp, int S, const void* sims, const double* vec, const double* dc,
                   const int* cube_idx, const double* weight, const int* cube_idx_host, double sim_res, int rx, int ry,
                   int rz, int Nsim, int Nx, int Ny, int Nz, int Nr, long long Npix, void* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Collectives of the sharded RIME step over RCCL (the replacement of DistributedLogProb.closure's per-device
 * Python loop, optim.py:1539-1566).  Thin wrappers: raw device pointers, the caller's stream, no allocation.
 * RCCL is resolved at first use (the copy already loaded into the process wins); without it every call
 * returns RIME_EUNSUPPORTED.  The shipped Python path drives the same RCCL operations through
 * torch.distributed; these give a host without torch.distributed the same two operations.
 *   rime_comm_unique_id : fills 128 bytes (ncclUniqueId) on ONE rank; the caller distributes them
 *   rime_comm_init      : ncclCommInitRank on the current device -> opaque communicator
 *   rime_comm_allgather_vis : every rank contributes `complex_per_rank` complex values (its block of the
 *       visibility tensor, blocks of equal size); vis_all receives nranks blocks in rank order
 *   rime_comm_reduce_grads  : in-place sum over ranks of `count` real values (gradients of replicated parameters)
 * ------------------------------------------------------------------------------------- */
int rime_comm_unique_id(void* id128);
int rime_comm_init(void** comm_out, int nranks, int rank, const void* id128);
int rime_comm_destroy(void* comm);
int rime_comm_allgather_vis(void* comm, int dtype, const void* vis_local, void* vis_all,
                            size_t complex_per_rank, void* stream);
int rime_comm_reduce_grads(void* comm, int dtype, void* grads, size_t count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RIME_HIP_H */
