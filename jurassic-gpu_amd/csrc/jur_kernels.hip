// jur_kernels.hip -- CDNA4 (gfx950) kernels of the JURASSIC EGA forward model.
//
//   jur_trace_kernel      one lane per ray: line-of-sight ray tracing through the 1-D
//                         atmosphere (reference algorithm: jr_common.h:585-711), writes the
//                         per-segment state p, T, ds, k, q_H2O, u[g] to the LOS workspace
//                         (tiles of 64 ray slots, [tile][point][field][64]), the tangent
//                         point, the point count and the surface temperature.
//   jur_track_trace_kernel  the same for a model with IP 2: every point and probe interpolated between the two
//                         nearest profiles of a satellite track (jurassic.c:704-760); writes the same workspace.
//   jur_cloud_trace_kernel  the same for a model with IP 3: every point and probe the distance-weighted mean over a
//                         cloud of air parcels (jurassic.c:763-804); writes the same workspace.
//   jur_ega_kernel        one lane per ray, one (channel, gas) pair per workgroup: the sequential
//                         emissivity-growth recurrence along the line of sight with its band
//                         table look-ups (jr_common.h:237-280); writes the gas's transmittance of the
//                         path up to and including every segment.
//   jur_cga_kernel        the same launch for a model with FORMOD 1: the Curtis-Godson means of the path so far as
//                         three running sums per lane (jr_common.h:455-473) and one table look-up at the means per
//                         segment; writes the same plane.
//   jur_combine_kernel    one lane per ray, one channel per workgroup: continua
//                         (jr_common.h:315-390), product over gases, Planck source (:220-224),
//                         radiance update (:293-300); surface term, brightness temperature and
//                         the NaN mask in the epilogue (CPUdrivers.c:5-24, jr_common.h:193-210).
//   jur_combine_group_kernel  the same with up to four channels of a ray block as the wavefronts of one
//                         workgroup (what runs when there is more than one channel).
//   Two table-search strategies in jur_ega_kernel: WARM (tables whose axes and curves are sorted: every
//   bracket is unique, so the search resumes from the bracket the previous segment ended in -- the
//   accumulated transmittance only falls, the column only grows) and EXACT (the reference's bisections
//   probe for probe, for unsorted tables).
//   jur_cg_kernel         optional: Curtis-Godson means along the path, one wavefront per (ray, gas)
//                         pencil, along-path prefix sums as wavefront scans (jr_common.h:455-473).
//   jur_raykey_kernel     geometric tangent altitude per ray; rays are then processed in
//                         that order (hipCUB radix sort) so that the lanes of a wavefront
//                         walk similar paths.
//   jur_pencil_kernel     package-sized calls: the whole path of a few rays in ONE workgroup -- a tracer wavefront,
//                         emissivity-growth wavefronts (lane per (ray, channel, gas) chain) and radiance-update
//                         wavefronts hand the line of sight on through rings in LDS while it is being traced; the
//                         same device functions as the three batched kernels, bit-identical results.
//   jur_fov_kernel        field-of-view convolution of device arrays (formod_fov, jurassic.c:214-258).
//   jur_scene_fov_kernel  the same convolution on the replicated rays of a pass of the scene entries, a workgroup per ray.
//   jur_scene_hydro_kernel  hydrostatic balance of the slices of a scene, one wavefront per segment (jur_model_set_scene_hydz).
//   jur_scene_gradient_kernel  b, cost and nlive of a scene's slices from held blocks, a lane per state element (jur_gradient_scene_host).
//   jur_scene_overflow_kernel  untraceable rays of a pass of the scene retrieval, a lane per slot, and
//   jur_scene_overflow_fold_kernel  their fold into NaN trial costs and failed slices (jur_model_set_scene_overflow).
//   jur_scene_gain_kernel  gain matrix G = S K^T W of a scene's slices over the ragged blocks, a workgroup per 64 x 64 tile;
//   jur_scene_budget_kernel  the row sums of G^2 var per error source, a lane per state element (jur_gain_scene_host).
//   jur_scene_cross_kernel  cross-state matrix C = G^T Kb of a scene's slices over the ragged blocks, a workgroup per 64 x 64 tile;
//   jur_scene_cross_pass_kernel  the same chains continued over the rays of one pass (jur_param_scene_host);
//   jur_scene_param_kernel  diag(C Sigma C^T) per parameter covariance, a workgroup per 64 rows of C (jur_param_slices_host).
//   jur_intpol_kernel     regridding of a track / point-cloud atmosphere (intpol_atm, jurassic.c:675-804).
//   jur_kat_*_kernel      known-answer hooks for tests: the device functions on arrays of inputs.
//
// All arithmetic is IEEE fp64; tables are fp32 in memory.  Compiled with -ffp-contract=off so that no fused
// multiply-adds are formed that the reference's x86-64 build does not form.
//   * Ray tracing, and the look-ups on tables that are not strictly increasing, keep the reference's operand order
//     throughout; where a division is replaced there (div_rcp, div_finite, div_const) the replacement returns the same
//     double as the division (tools/compare_builds.py).
//   * Since round 3 the look-up on strictly increasing tables (every table that passes the reference's row rule) and the
//     radiance update spend part of the contract's tolerance -- 1e-6 relative on radiances, 1e-9 in the test suite -- on
//     cheaper arithmetic: curve interpolations through bracket slopes formed once per model, blends through reciprocal
//     widths, the path transmittance carried as 1 - eps, one shared 1/T, exp through a table, tanh through exp
//     (lip_slope, lip_mulr, rcp_t, exp_tab, tanh_pos, segment_tau_gas below say what each costs in accuracy): 6e-12
//     relative on radiances against the bit-exact build.  The bit-exact look-ups remain as known-answer modes (jur_kat_ega_eps, modes 0 .. 2).

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <cstdlib>
#include <mutex>
#include "jur_internal.h"

#define NLOS JUR_NLOS
#define TBLNS JUR_TBLNS

namespace {

// ---------------------------------------------------------------------------------------
// small helpers (jr_common.h:43-57)
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double c01(double x) { return (x > 1.) ? 1. : ((x < 0.) ? 0. : x); }
// the same clamp for an x that is known not to be NaN (v_min_f64 / v_max_f64 return the other operand for a
// NaN, the comparisons above return the NaN): 2 instructions instead of 6.  No caller is left since fma_c01 / add_c01
// below; it stays as the definition of what those two compute.
__device__ __forceinline__ double c01_num(double x) { return __builtin_fmax(__builtin_fmin(x, 1.), 0.); }
// c01_num folded into the instruction that produces x: the VOP3 `clamp` output modifier clamps the rounded fp64 result
// to [0, 1], for every non-NaN x the very double min(max(x, 0), 1) -- and no instruction of its own, where c01_num is two
// at the fp64 rate.  (The compiler does not form the modifier here: without fast-math the fold needs a no-NaN
// guarantee.)  What the modifier makes of a NaN depends on the kernel's DX10-clamp mode (0 with it, the NaN without);
// that does not matter where these are used: the strict-table look-up answers NaN inputs before it reaches a clamp, and
// the tables hold none.  The one value the two forms could give differently is a zero's sign (x = -0).  No table rule is
// needed against that: a clamp's result is only ever added to, subtracted from or multiplied, a zero of either sign gives
// the same non-zero results there and at most another zero of either sign, and what the look-up hands on is
// 1 - eps_t = 1 for both -- the sign of a zero never reaches an output.
__device__ __forceinline__ double fma_c01(double a, double b, double c) {      // c01_num(fma(a, b, c))
  double d;
  asm volatile("v_fma_f64 %0, %1, %2, %3 clamp" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
__device__ __forceinline__ double add_c01(double a, double b) {                // c01_num(a + b)
  double d;
  asm volatile("v_add_f64 %0, %1, %2 clamp" : "=v"(d) : "v"(a), "v"(b));
  return d;
}

__device__ __forceinline__ double lip(double x0, double y0, double x1, double y1, double x) {
  return y0 + (x - x0) * (y1 - y0) / (x1 - x0);
}

// The same interpolation with the bracket width's reciprocal r = RN(1/(x1 - x0)) at hand.  The quotient
// a/b is formed as q = RN(a r), q' = RN(q + (a - b q) r) with fused multiply-adds: q' is the correctly
// rounded a/b (Markstein 1990: r correctly rounded and q faithful suffice), i.e. the very double the
// division returns, for 3 instructions instead of the ~14 of an fp64 division.  Needs b != 0 and finite.
__device__ __forceinline__ double div_rcp(double a, double b, double r) {
  double const q = a * r;
  return __builtin_fma(__builtin_fma(-b, q, a), r, q);
}
__device__ __forceinline__ double lip_rcp(double x0, double y0, double x1, double y1, double x, double r) {
  return y0 + div_rcp((x - x0) * (y1 - y0), x1 - x0, r);
}

// a / b for finite a and finite b != 0 whose exponents are nowhere near the ends of the fp64 range
// (bracket widths of validated tables, emissivities, column densities, 1e-9 <= tau <= 1): the compiler's
// fp64 division is rcp + two Newton steps + quotient + residual correction, wrapped in v_div_scale /
// v_div_fmas (exponent rescaling) and v_div_fixup (zero, infinity, NaN, denormal results).  For such
// operands the wrapping is the identity, so the bare sequence returns the same double in 8 instead of
// 11 instructions.
__device__ __forceinline__ double div_finite(double a, double b) {
  double r = __builtin_amdgcn_rcp(b);
  r = __builtin_fma(r, __builtin_fma(-b, r, 1.0), r);
  r = __builtin_fma(r, __builtin_fma(-b, r, 1.0), r);
  double const q = a * r;
  return __builtin_fma(__builtin_fma(-b, q, a), r, q);
}
__device__ __forceinline__ double lip_finite(double x0, double y0, double x1, double y1, double x) {
  return y0 + div_finite((x - x0) * (y1 - y0), x1 - x0);
}

// ---- arithmetic of the strict-table path (round 3) -------------------------------------------------------------
// The contract is 1e-6 relative on the radiances and the suite holds 1e-9; bit-identity with the reference's
// divisions is not needed to stay 1e3 .. 1e6 times inside that, and it is what 40 % of the look-up's fp64 work went
// into.  On tables whose axes and curves are strictly increasing (no zero-width bracket) the look-up uses:
//   lip_slope  the eight curve interpolations as y0 + (x - x0) s, one fused multiply-add, with the bracket's slope s
//              read from the bracket's record (jur_records_kernel: the correctly rounded quotient of the bracket's fp64
//              differences, formed once per model) where rounds 1 - 2 divided (8 instructions) and the first round-3 version
//              multiplied with a Newton-refined v_rcp_f64 (4, and the difference y1 - y0): good to an ulp or two of
//              the interpolated value;
//   lip_mulr   the p and T blends as y0 + ((x - x0) (y1 - y0)) r with r = RN(1 / (x1 - x0)): two roundings instead
//              of the division's one, 1 instruction instead of 3;
//   the path transmittance is carried as tau <- 1 - eps_t instead of tau <- tau * ((1 - eps_t) / tau): the same
//   number up to the two roundings the reference spends on dividing by tau and multiplying with it again (the
//   radiance update divides the products over the gases of consecutive segments instead: one division per
//   (channel, segment) in place of one per (channel, gas, segment)).
// tests/test_kat_gpu.py holds this path against the bit-exact ones (modes 0 .. 2), which stay the known-answer
// reference on the device.
__device__ __forceinline__ double lip_slope(double x0, double y0, double s, double x) { return __builtin_fma(x - x0, s, y0); }
__device__ __forceinline__ double lip_mulr(double x0, double y0, double y1, double x, double r) {
  return y0 + ((x - x0) * (y1 - y0)) * r;
}
// c01_num of the two, clamped by their last instruction (fma_c01 / add_c01): the same doubles
__device__ __forceinline__ double lip_slope_c01(double x0, double y0, double s, double x) { return fma_c01(x - x0, s, y0); }
__device__ __forceinline__ double lip_mulr_c01(double x0, double y0, double y1, double x, double r) {
  return add_c01(y0, ((x - x0) * (y1 - y0)) * r);
}

// exp(x) of the radiance update and the continua (round 3).  The device library's exp is a degree-11 polynomial whose
// eleven coefficients the compiler keeps in 22 VGPRs across the segment loop and copies in front of every Horner
// step (v_mov_b64 + v_fmac_f64): ~35 vector instructions per call, three to four calls per (segment, channel).  This
// one reduces x = (64 m + j) ln2/64 + r, |r| <= ln2/128, takes 2^(j/64) from a 64-entry table (correctly rounded
// doubles; in LDS in the batched kernels) and needs a degree-5 polynomial in r (remainder r^6/720 < 4e-17):
// 17 vector instructions and one table read, within ~1 ulp of the library's result -- 1e-16 relative where the
// contract is 1e-6.  |x| is clamped to 1000 (beyond +-745 the result is 0 or inf either way), NaN goes through.
__device__ const double JUR_EXP2_64[64] = {
  1.0, 1.0108892860517005, 1.0218971486541166, 1.0330248790212284,
  1.0442737824274138, 1.0556451783605572, 1.0671404006768237, 1.0787607977571199,
  1.0905077326652577, 1.102382583307841, 1.1143867425958924, 1.1265216186082418,
  1.1387886347566916, 1.1511892299529827, 1.1637248587775775, 1.1763969916502812,
  1.189207115002721, 1.202156731452703, 1.215247359980469, 1.22848053610687,
  1.241857812073484, 1.255380757024691, 1.2690509571917332, 1.2828700160787783,
  1.2968395546510096, 1.3109612115247644, 1.3252366431597413, 1.339667524053303,
  1.3542555469368927, 1.3690024229745905, 1.383909881963832, 1.3989796725383112,
  1.4142135623730951, 1.42961333839197, 1.4451808069770467, 1.460917794180647,
  1.4768261459394993, 1.4929077282912648, 1.5091644275934228, 1.5255981507445384,
  1.5422108254079407, 1.559004400237837, 1.5759808451078865, 1.593142151342267,
  1.6104903319492543, 1.6280274218573478, 1.645755478153965, 1.6636765803267364,
  1.681792830507429, 1.7001063537185235, 1.718619298122478, 1.7373338352737062,
  1.7562521603732995, 1.7753764925265212, 1.7947090750031072, 1.8142521755003989,
  1.8340080864093424, 1.8539791250833855, 1.8741676341103, 1.8945759815869656,
  1.9152065613971474, 1.9360617934922943, 1.9571441241754002, 1.978456026387951};

template <class Tab>
__device__ __forceinline__ double exp_tab(Tab const &tab, double x) {
  double const xc = __builtin_fmin(__builtin_fmax(x, -1000.), 1000.);
  double const k = __builtin_rint(xc * 92.33248261689366);              // 64 / ln 2
  int const n = (int)k;
  double r = __builtin_fma(k, -0.01083042468962958, xc);                // ln2/64, upper bits (trailing zeros: exact)
  r = __builtin_fma(k, -6.619564634077006e-12, r);                      // ... and the rest
  double q = __builtin_fma(r, 1. / 120, 1. / 24);
  q = __builtin_fma(q, r, 1. / 6);
  q = __builtin_fma(q, r, 0.5);
  q = __builtin_fma(q * r, r, r);                                       // e^r - 1
  double const t = tab[n & 63];
  double const res = __builtin_ldexp(__builtin_fma(t, q, t), n >> 6);
  return (x != x) ? x : res;
}
// the table where a kernel has no copy in LDS
struct Exp2Global { __device__ __forceinline__ double operator[](int j) const { return JUR_EXP2_64[j]; } };
struct Exp2Lds { double const *t; __device__ __forceinline__ double operator[](int j) const { return t[j]; } };

// bracket search on an ascending or descending axis (jr_common.h:87-104); P: a pointer to doubles in global memory
// or (lds_cptr, the tracer's staged profile slice) in LDS
template <class P>
__device__ __forceinline__ int locate_axis(P xx, int n, double x) {
  int ilo = 0, ihi = n - 1, i = (n - 1) >> 1;
  if (xx[i] < xx[i + 1]) {
    while (ihi > ilo + 1) {
      i = (ihi + ilo) >> 1;
      if (xx[i] > x) ihi = i; else ilo = i;
    }
  } else {
    while (ihi > ilo + 1) {
      i = (ihi + ilo) >> 1;
      if (xx[i] <= x) ihi = i; else ilo = i;
    }
  }
  return ilo;
}

// ---------------------------------------------------------------------------------------
// geometry (jr_common.h:475-500)
// ---------------------------------------------------------------------------------------
#define JUR_PI 3.14159265358979323846
#define RAD2GRD (180 / JUR_PI)
#define GRD2RAD (JUR_PI / 180)

__device__ __forceinline__ double norm3(double const x[3]) { return sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]); }

__device__ __forceinline__ void cart2geo(double const x[3], double &alt, double &lon, double &lat) {
  double const radius = norm3(x);
  lat = asin(x[2] / radius) * RAD2GRD;
  lon = atan2(x[1], x[0]) * RAD2GRD;
  alt = radius - JUR_RE;
}

__device__ __forceinline__ void geo2cart(double alt, double lon, double lat, double x[3]) {
  double const radius = alt + JUR_RE, clat = cos(lat * GRD2RAD);
  x[0] = radius * clat * cos(lon * GRD2RAD);
  x[1] = radius * clat * sin(lon * GRD2RAD);
  x[2] = radius * sin(lat * GRD2RAD);
}

__device__ __forceinline__ double refractivity(double p, double t) { return 7.753e-05 * p / t; }

// Same bracket as locate_axis for a sorted axis, found by walking from a guess (the previous
// point's bracket: altitude changes by <= RAYDZ per step).  dir > 0 ascending, < 0 descending.
template <class P>
__device__ __forceinline__ int locate_axis_from(P xx, int n, double x, int dir, int g) {
  int i = min(max(g, 0), n - 2);
  if (dir > 0) {
    while (i > 0 && xx[i] > x) --i;
    while (i < n - 2 && !(xx[i + 1] > x)) ++i;
  } else {
    while (i > 0 && xx[i] <= x) --i;
    while (i < n - 2 && !(xx[i + 1] <= x)) ++i;
  }
  return i;
}

// pressure and temperature of the profile slice [i0, i0+n) at altitude z0 (jr_common.h:549-555);
// `hint` carries the bracket from call to call (dir == 0: exact bisection, axis not sorted).
// WANT_R: the caller interpolates more quantities on the same bracket; for a sorted axis (dir != 0: z strictly
// monotone, bracket width non-zero) it gets rdz = RN(1 / (zb - za)) and every such interpolation, the
// temperature's included, divides through it (lip_rcp: the same doubles, 3 instructions per quotient).
//
// Where the tracer reads the profile rows from.  AtmGlobal: the model's arrays, indexed by atmosphere point.  AtmLds:
// the rows z, p, T, pslope, q[ng], k[nw] of ONE slice, n levels each, staged in LDS by the workgroup and indexed from
// the slice's first level -- pointers typed as LDS, so that every read is a ds_read (counted on lgkmcnt alone: a
// read through a generic pointer to the same bytes is a flat_load, which also waits in vmcnt behind the LOS stores).
// origin(atm0): index of the slice's first level in the rows.
typedef __attribute__((address_space(3))) double const *lds_cptr;
struct AtmGlobal {
  typedef double const *ptr;
  static constexpr bool track = false;   // one profile per time block (ip == 1); AtmTrack: the nearest two of a track
  static constexpr bool cloud = false;   // AtmCloud: the weighted mean over the block's point cloud (ip == 3)
  jur_view_t const &v;
  __device__ __forceinline__ ptr z() const { return v.atm_z; }
  __device__ __forceinline__ ptr p() const { return v.atm_p; }
  __device__ __forceinline__ ptr t() const { return v.atm_t; }
  __device__ __forceinline__ ptr pslope() const { return v.atm_pslope; }
  __device__ __forceinline__ ptr q(int ig) const { return v.atm_q + (size_t)ig * v.atm_np; }
  __device__ __forceinline__ ptr k(int iw) const { return v.atm_k + (size_t)iw * v.atm_np; }
  __device__ __forceinline__ int origin(int atm0) const { return atm0; }
};
struct AtmLds {
  typedef lds_cptr ptr;
  static constexpr bool track = false;
  static constexpr bool cloud = false;
  lds_cptr rows;
  int n, ng;
  __device__ __forceinline__ ptr z() const { return rows; }
  __device__ __forceinline__ ptr p() const { return rows + n; }
  __device__ __forceinline__ ptr t() const { return rows + 2 * n; }
  __device__ __forceinline__ ptr pslope() const { return rows + 3 * n; }
  __device__ __forceinline__ ptr q(int ig) const { return rows + (4 + ig) * n; }
  __device__ __forceinline__ ptr k(int iw) const { return rows + (4 + ng + iw) * n; }
  __device__ __forceinline__ int origin(int) const { return 0; }
};

template <bool WANT_R = false, class Atm>
__device__ __forceinline__ int intpol_pt(Atm const &A, int i0, int n, double z0, double &p, double &t, int dir,
                                         int &hint, double *rdz = nullptr) {
  typename Atm::ptr const az = A.z(), ap = A.p(), at = A.t();
  int const loc = dir ? locate_axis_from(az + i0, n, z0, dir, hint) : locate_axis(az + i0, n, z0);
  hint = loc;
  int const ip = i0 + loc;
  double const za = az[ip], zb = az[ip + 1];
  // eip (jr_common.h:53-57) with log(p1/p0)/(z1-z0) taken from the per-level array that
  // jur_pslope_kernel filled with exactly that expression; NaN marks a non-positive pressure
  double const sl = A.pslope()[ip];
  if (WANT_R && dir) {
    double const r = 1. / (zb - za);
    *rdz = r;
    p = (sl == sl) ? ap[ip] * exp(sl * (z0 - za)) : lip_rcp(za, ap[ip], zb, ap[ip + 1], z0, r);
    t = lip_rcp(za, at[ip], zb, at[ip + 1], z0, r);
  } else {
    p = (sl == sl) ? ap[ip] * exp(sl * (z0 - za)) : lip(za, ap[ip], zb, ap[ip + 1], z0);
    t = lip(za, at[ip], zb, at[ip + 1], z0);
  }
  return ip;
}

// once per atmosphere upload: slope of ln p between neighbouring levels, as eip forms it
__global__ void jur_pslope_kernel(int n, double const *__restrict__ z, double const *__restrict__ p,
                                  double *__restrict__ slope) {
  int const i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = __builtin_nan("");
  if (i + 1 < n) {
    double const y0 = p[i], y1 = p[i + 1];
    if ((y0 > 0) && (y1 > 0)) s = log(y1 / y0) / (z[i + 1] - z[i]);
  }
  slope[i] = s;
}

// ---------------------------------------------------------------------------------------
// ray tracing, one lane per ray
// ---------------------------------------------------------------------------------------
// Exit clipping (jr_common.h:637-648), once per ray: the previous point is rebuilt from its geodetic
// coordinates and the last segment is cut at the atmosphere's boundary.  Kept out of line: inlined, the
// asin/atan2/sin/cos polynomials have their ~40 constants hoisted in front of the stepping loop, where
// they cost the loop its registers (spills whose reloads queue behind the LOS stores).
// The point before the exit gets its segment length only when the exit is found (jr_common.h:645-646):
// its trapezoid weight and column densities, written provisionally one step earlier, are redone here from
// the same profile bracket (same inputs, same doubles).  Out of line, once per ray.
__device__ __attribute__((noinline)) void redo_columns(double const *__restrict__ atm_z, double const *__restrict__ atm_q,
                                                       int atm_np, int i0, int n, int ng, double z, double p, double t,
                                                       double dsn, double *__restrict__ los_u, size_t fs) {
  int const ip = i0 + locate_axis(atm_z + i0, n, z);
  double const za = atm_z[ip], zb = atm_z[ip + 1];
  for (int ig = 0; ig < ng; ig++) {
    double const *q = atm_q + (size_t)ig * atm_np;
    los_u[(size_t)ig * fs] = 10. * lip(za, q[ip], zb, q[ip + 1], z) * p / (JUR_BOLTZMANN * t) * dsn;
  }
}

// ---------------------------------------------------------------------------------------
// 2-D atmosphere along the line of sight (ctl->ip == 2: intpol_atm_2d, jurassic.c:704-760; the rule in jurassic_hip.h)
// ---------------------------------------------------------------------------------------
// Where the profile table of a ray's time block is read from.  TrackGlobal: the model's table (jur_track_t), indexed by
// profile.  TrackLds: the workgroup's copy of ONE block's nx entries in LDS -- columns x1[0], x1[1], x1[2], lat as
// doubles, then first, len, dir as ints -- indexed by profile all the same (the block's first profile is px0).
typedef __attribute__((address_space(3))) int const *lds_iptr;
struct TrackGlobal {
  double const *x1_, *lat_;
  int const *first_, *len_, *dir_;
  __device__ __forceinline__ double x1(int ix, int i) const { return x1_[3 * (size_t)ix + i]; }
  __device__ __forceinline__ double lat(int ix) const { return lat_[ix]; }
  __device__ __forceinline__ int first(int ix) const { return first_[ix]; }
  __device__ __forceinline__ int len(int ix) const { return len_[ix]; }
  __device__ __forceinline__ int dir(int ix) const { return dir_[ix]; }
};
struct TrackLds {
  lds_cptr d;
  lds_iptr w;
  int px0, nx;
  __device__ __forceinline__ double x1(int ix, int i) const { return d[i * nx + (ix - px0)]; }
  __device__ __forceinline__ double lat(int ix) const { return d[3 * nx + (ix - px0)]; }
  __device__ __forceinline__ int first(int ix) const { return w[ix - px0]; }
  __device__ __forceinline__ int len(int ix) const { return w[nx + (ix - px0)]; }
  __device__ __forceinline__ int dir(int ix) const { return w[2 * nx + (ix - px0)]; }
};
// the profile rows come from the model's arrays, as under AtmGlobal
template <class Tab>
struct AtmTrack {
  typedef double const *ptr;
  static constexpr bool track = true;
  static constexpr bool cloud = false;
  jur_view_t const &v;
  Tab T;
  int const *prof_of;
  __device__ __forceinline__ ptr z() const { return v.atm_z; }
  __device__ __forceinline__ ptr p() const { return v.atm_p; }
  __device__ __forceinline__ ptr t() const { return v.atm_t; }
  __device__ __forceinline__ ptr pslope() const { return v.atm_pslope; }
  __device__ __forceinline__ ptr q(int ig) const { return v.atm_q + (size_t)ig * v.atm_np; }
  __device__ __forceinline__ ptr k(int iw) const { return v.atm_k + (size_t)iw * v.atm_np; }
  __device__ __forceinline__ int origin(int atm0) const { return atm0; }
};

// latitude of a position and x0 = geo2cart(0, lon, lat) of its longitude and latitude (jurassic.c:731), in upstream's
// order of operations.  Out of line for the reason clip_exit is: five evaluations per step would each bring the
// constants of asin, atan2, sin and cos in front of the stepping loop.
struct TrackGeo { double lat, x0, x1, x2; };
__device__ __attribute__((noinline)) TrackGeo track_geo(double px0, double px1, double px2) {
  double const x[3] = {px0, px1, px2};
  double alt, lon, lat, c[3];
  cart2geo(x, alt, lon, lat);
  geo2cart(0, lon, lat, c);
  return {lat, c[0], c[1], c[2]};
}

// What a point takes from the track: its two neighbour profiles (table index), the lower point of its altitude
// bracket in either, and the weight r of the second.  A ray carries one for its LOS points and one for its probes:
// the brackets are the hints of the next evaluation while the neighbour stays (ix < 0: nothing carried yet).
struct TrackPt { int ix0, ix1, i0, i1; double r; };

// jurassic.c:732-755 on the profiles [px0, px0 + nx) of the ray's block: the full scan, upstream's comparisons and
// order; then the bracket locate() finds on either profile's own levels (walked from the hint where the profile's
// axis is strictly monotone: the same bracket)
template <class Tab>
__device__ __forceinline__ TrackPt track_locate(Tab const &T, double const *__restrict__ atm_z, int px0, int nx, double z,
                                                TrackGeo const &g, TrackPt const &prev) {
  double dhmin0 = 1e99, dhmin1 = 1e99;
  int ix0 = px0, ix1 = px0;
  for (int ix = px0; ix < px0 + nx; ix++)
    if (fabs(g.lat - T.lat(ix)) <= 10) {
      double const a0 = g.x0 - T.x1(ix, 0), a1 = g.x1 - T.x1(ix, 1), a2 = g.x2 - T.x1(ix, 2);
      double const dh = a0 * a0 + a1 * a1 + a2 * a2;
      if (dh <= dhmin0) { dhmin1 = dhmin0; ix1 = ix0; dhmin0 = dh; ix0 = ix; }
      else if (dh <= dhmin1) { dhmin1 = dh; ix1 = ix; }
    }
  double const b0 = T.x1(ix0, 0) - T.x1(ix1, 0), b1 = T.x1(ix0, 1) - T.x1(ix1, 1), b2 = T.x1(ix0, 2) - T.x1(ix1, 2);
  double const x2 = b0 * b0 + b1 * b1 + b2 * b2;
  double const x = sqrt(x2);
  double const r0 = (dhmin0 - dhmin1 + x2) / (2 * x);
  double const r1 = x - r0;
  double r;
  if (r0 <= 0) r = 0;
  else r = (r1 <= 0) ? 1 : r0 / (r0 + r1);
  int const f0 = T.first(ix0), f1 = T.first(ix1), d0 = T.dir(ix0), d1 = T.dir(ix1);
  int const h0 = (ix0 == prev.ix0) ? prev.i0 - f0 : (ix0 == prev.ix1) ? prev.i1 - f0 : 0;
  int const h1 = (ix1 == prev.ix1) ? prev.i1 - f1 : (ix1 == prev.ix0) ? prev.i0 - f1 : 0;
  int const l0 = d0 ? locate_axis_from(atm_z + f0, T.len(ix0), z, d0, h0) : locate_axis(atm_z + f0, T.len(ix0), z);
  int const l1 = d1 ? locate_axis_from(atm_z + f1, T.len(ix1), z, d1, h1) : locate_axis(atm_z + f1, T.len(ix1), z);
  return {ix0, ix1, f0 + l0, f1 + l1, r};
}

__device__ __forceinline__ double track_mix(double r, double y0, double y1) { return (1 - r) * y0 + r * y1; }

// pressure (eip through the pslope array) and temperature (lip) of either profile on its bracket, then blended
template <class Atm>
__device__ __forceinline__ void track_pt(Atm const &A, TrackPt const &k, double z, double &p, double &t) {
  double pj[2], tj[2];
  for (int j = 0; j < 2; j++) {
    int const i = j ? k.i1 : k.i0;
    double const za = A.z()[i], zb = A.z()[i + 1], sl = A.pslope()[i];
    pj[j] = (sl == sl) ? A.p()[i] * exp(sl * (z - za)) : lip(za, A.p()[i], zb, A.p()[i + 1], z);
    tj[j] = lip(za, A.t()[i], zb, A.t()[i + 1], z);
  }
  p = track_mix(k.r, pj[0], pj[1]);
  t = track_mix(k.r, tj[0], tj[1]);
}

// one row (an emitter's q, a window's k) at altitude z on the point's two brackets, blended
__device__ __forceinline__ double track_row(double const *__restrict__ az, double const *__restrict__ y, TrackPt const &k, double z) {
  return track_mix(k.r, lip(az[k.i0], y[k.i0], az[k.i0 + 1], y[k.i0 + 1], z), lip(az[k.i1], y[k.i1], az[k.i1 + 1], y[k.i1 + 1], z));
}

// redo_columns under the 2-D rule: the point before the exit at position (px0, px1, px2), altitude z
template <class Tab>
__device__ __attribute__((noinline)) void redo_columns_track(Tab T, double const *__restrict__ atm_z, double const *__restrict__ atm_q,
                                                             int atm_np, int px0, int nx, int ng, double x0, double x1, double x2,
                                                             double z, double p, double t, double dsn, double *__restrict__ los_u,
                                                             size_t fs) {
  TrackGeo const g = track_geo(x0, x1, x2);
  TrackPt const k = track_locate(T, atm_z, px0, nx, z, g, TrackPt{-1, -1, 0, 0, 0.});
  for (int ig = 0; ig < ng; ig++)
    los_u[(size_t)ig * fs] = 10. * track_row(atm_z, atm_q + (size_t)ig * atm_np, k, z) * p / (JUR_BOLTZMANN * t) * dsn;
}

// ---------------------------------------------------------------------------------------
// point-cloud atmosphere along the line of sight (ctl->ip == 3: intpol_atm_3d, jurassic.c:763-804; the rule in
// jurassic_hip.h)
// ---------------------------------------------------------------------------------------
// Where the gate columns of a ray's cloud -- altitude, latitude and cached position of every point of its time block --
// are read from, indexed by atmosphere point in either case.  CloudGlobal: the model's rows and its position table
// (jur_cloud_t).  CloudLds: the workgroup's copy of ONE block [a0, a0 + n) in LDS, columns z, lat, x1[0], x1[1], x1[2]
// of n doubles each, with the block's altitude range, which the workgroup reduced while it staged.
struct CloudGlobal {
  static constexpr bool staged = false;
  double const *z_, *lat_, *x1_;
  __device__ __forceinline__ double z(int ip) const { return z_[ip]; }
  __device__ __forceinline__ double lat(int ip) const { return lat_[ip]; }
  __device__ __forceinline__ double x1(int ip, int i) const { return x1_[3 * (size_t)ip + i]; }
};
struct CloudLds {
  static constexpr bool staged = true;
  lds_cptr d;
  int a0, n;
  double zmin, zmax;
  __device__ __forceinline__ double z(int ip) const { return d[ip - a0]; }
  __device__ __forceinline__ double lat(int ip) const { return d[n + (ip - a0)]; }
  __device__ __forceinline__ double x1(int ip, int i) const { return d[(2 + i) * n + (ip - a0)]; }
};
// the values p, T, q, k come from the model's rows, for the points that pass the gates
template <class Tab>
struct AtmCloud {
  typedef double const *ptr;
  static constexpr bool track = false;
  static constexpr bool cloud = true;
  jur_view_t const &v;
  Tab T;
  double cx, cz;
  __device__ __forceinline__ int origin(int atm0) const { return atm0; }
};

// jurassic.c:778-792 on the points [a0, a0 + n), in ascending index: the three gates, the weight, wsum; hit(ip, w)
// takes a point that contributes.  Every product and sum is rounded on its own (no contraction), every quotient is a
// true division.
template <class Tab, class F>
__device__ __forceinline__ double cloud_scan(Tab const &T, int a0, int n, double cx, double cz, double z0, TrackGeo const &g,
                                             F &&hit) {
#pragma clang fp contract(off)
  double const rm2 = cx * cx;
  double wsum = 0;
  for (int ip = a0; ip < a0 + n; ip++) {
    double const dz = fabs(T.z(ip) - z0);
    if (dz >= cz) continue;
    if (fabs(T.lat(ip) - g.lat) * 111.13 >= cx) continue;
    double const b0 = g.x0 - T.x1(ip, 0), b1 = g.x1 - T.x1(ip, 1), b2 = g.x2 - T.x1(ip, 2);
    double const dx2 = b0 * b0 + b1 * b1 + b2 * b2;
    if (dx2 >= rm2) continue;
    double const w = (1 - dz / cz) * (rm2 - dx2) / (rm2 + dx2);
    wsum += w;
    hit(ip, w);
  }
  return wsum;
}

// the rows a point can take from the model's arrays: 0 p, 1 T, 2 .. q[ng], then k[nw]
struct CloudRows {
  double const *p, *t, *q, *k;
  int atm_np, ng, nw;
  __device__ __forceinline__ double const *row(int r) const {
    return (r == 0) ? p : (r == 1) ? t : (r < 2 + ng) ? q + (size_t)(r - 2) * atm_np : k + (size_t)(r - 2 - ng) * atm_np;
  }
};
struct CloudPT { double p, t; };

// rule 4 for pressure and temperature alone (the refraction probes): jurassic.c:794-803 after the scan
template <class Tab>
__device__ __forceinline__ CloudPT cloud_mean_pt(Tab const &T, CloudRows const &R, int a0, int n, double cx, double cz, double z0,
                                                 TrackGeo const &g) {
#pragma clang fp contract(off)
  double p = 0, t = 0;
  double const wsum = cloud_scan(T, a0, n, cx, cz, z0, g, [&](int ip, double w) { p += w * R.p[ip]; t += w * R.t[ip]; });
  if (wsum >= 1e-6) { p /= wsum; t /= wsum; }
  else p = t = __builtin_nan("");
  return {p, t};
}

// rule 4 for every row: y[0] p, y[1] T, y[2 ..] q[ng], k[nw] (2 + ng + nw doubles)
template <class Tab>
__device__ __forceinline__ void cloud_mean_all(Tab const &T, CloudRows const &R, int a0, int n, double cx, double cz, double z0,
                                               TrackGeo const &g, double *__restrict__ y) {
#pragma clang fp contract(off)
  int const nrow = 2 + R.ng + R.nw;
  for (int r = 0; r < nrow; r++) y[r] = 0;
  double const wsum = cloud_scan(T, a0, n, cx, cz, z0, g, [&](int ip, double w) {
    for (int r = 0; r < nrow; r++) y[r] += w * R.row(r)[ip];
  });
  if (wsum >= 1e-6) for (int r = 0; r < nrow; r++) y[r] /= wsum;
  else for (int r = 0; r < nrow; r++) y[r] = __builtin_nan("");
}

// The two evaluations of the tracer, out of line as track_geo and clip_exit are: a probe (p, T) and a LOS point (every
// row) at the position (px0, px1, px2), altitude z0.  Five scans a step, each over the whole cloud of the block.
template <class Tab>
__device__ __attribute__((noinline)) CloudPT cloud_probe(Tab T, double const *__restrict__ ap, double const *__restrict__ at, int a0,
                                                         int n, double cx, double cz, double px0, double px1, double px2,
                                                         double z0) {
  return cloud_mean_pt(T, CloudRows{ap, at, nullptr, nullptr, 0, 0, 0}, a0, n, cx, cz, z0, track_geo(px0, px1, px2));
}
template <class Tab>
__device__ __attribute__((noinline)) void cloud_point(Tab T, double const *__restrict__ ap, double const *__restrict__ at,
                                                      double const *__restrict__ aq, double const *__restrict__ ak, int atm_np,
                                                      int ng, int nw, int a0, int n, double cx, double cz, double px0, double px1,
                                                      double px2, double z0, double *__restrict__ y) {
  cloud_mean_all(T, CloudRows{ap, at, aq, ak, atm_np, ng, nw}, a0, n, cx, cz, z0, track_geo(px0, px1, px2), y);
}

// redo_columns under the 3-D rule: the point before the exit at position (px0, px1, px2), altitude z
template <class Tab>
__device__ __attribute__((noinline)) void redo_columns_cloud(Tab T, double const *__restrict__ ap, double const *__restrict__ at,
                                                             double const *__restrict__ aq, double const *__restrict__ ak,
                                                             int atm_np, int ng, int nw, int a0, int n, double cx, double cz,
                                                             double px0, double px1, double px2, double z, double p, double t,
                                                             double dsn, double *__restrict__ los_u, size_t fs) {
  double y[2 + JUR_NG + JUR_NW];
  cloud_mean_all(T, CloudRows{ap, at, aq, ak, atm_np, ng, nw}, a0, n, cx, cz, z, track_geo(px0, px1, px2), y);
  for (int ig = 0; ig < ng; ig++) los_u[(size_t)ig * fs] = 10. * y[2 + ig] * p / (JUR_BOLTZMANN * t) * dsn;
}

struct ClipOut { double x0, x1, x2, frac; };
__device__ __attribute__((noinline)) ClipOut clip_exit(double px0, double px1, double px2, double pz, double x0, double x1,
                                                       double x2, double z, double zfrac) {
  double const px[3] = {px0, px1, px2};
  double xh[3], pzz, plon, plat;
  cart2geo(px, pzz, plon, plat);   // == the previous point's stored geolocation upstream
  geo2cart(pz, plon, plat, xh);
  double const frac = (zfrac - pz) / (z - pz);
  return {xh[0] + frac * (x0 - xh[0]), xh[1] + frac * (x1 - xh[1]), xh[2] + frac * (x2 - xh[2]), frac};
}

#define TR_PZ tr_sh[0][threadIdx.x & 63]
#define TR_PX(i) tr_sh[1 + (i)][threadIdx.x & 63]
#define TR_LZ0 tr_sh[4][threadIdx.x & 63]
#define TR_LX0(i) tr_sh[5 + (i)][threadIdx.x & 63]
#define TR_LZ1 tr_sh[8][threadIdx.x & 63]
#define TR_LDS1 tr_sh[9][threadIdx.x & 63]
#define TR_LZ2 tr_sh[10][threadIdx.x & 63]
#define TR_LX2(i) tr_sh[11 + (i)][threadIdx.x & 63]
#define TR_LDS2 tr_sh[14][threadIdx.x & 63]
// value of lane K of the caller's quad (lanes 4q .. 4q+3), for all four lanes: two DPP moves
template <int K>
__device__ __forceinline__ double quad_bcast(double x) {
  constexpr int ctrl = K | (K << 2) | (K << 4) | (K << 6);               // quad_perm:[K,K,K,K]
  int const lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), ctrl, 0xf, 0xf, false);
  int const hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), ctrl, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// One line of sight (traceray, jr_common.h:585-711, with tangent_point :502-539, trapezoid_rule_pos :437-443 and
// column_density :446-453 folded in), one lane per ray.  L says where the LOS fields of a point live -- the HBM
// workspace of the batched kernels, or a ring in LDS in the fused kernel -- through
//   L.at(field, point)      reference to the field's slot;  L.put(field, point, x) writes it
//   L.field_stride()        distance between the slots of consecutive fields (the emitters' columns are consecutive)
//   L.begin_point(i)        called before point i is first written
//   L.points_final(i)       called when points 0 .. i-1 will not change any more (point i still may: the exit
//                           clipping rewrites the point before the exit, jr_common.h:645-646)
//   L.never_enter(mask)     called once by all lanes together: the lanes whose rays never enter the atmosphere
//   L.ray_final(n, tsurf)   called when the ray has left the atmosphere with n points, all final (not for a ray
//                           that runs into the NLOS limit: see the returned np)
// tr_sh: the per-lane tangent-point bookkeeping of the caller's wavefront in LDS, column threadIdx.x & 63.
// A: where the profile rows are read from in the stepping loop (AtmGlobal / AtmLds).  What a ray reads once -- the
// slice search, the altitude range, redo_columns -- goes to the model's arrays in either case.
// QUAD: the ray is traced by the four lanes of a quad together (fused kernel, where the tracer wavefront has lanes
// to spare and the call's latency is the tracer's dependent instruction chain).  All four run the step
// redundantly -- same inputs, same doubles -- except for the refractivity gradient (jr_common.h:665-681), 58 % of
// the step's instructions: lane 0 takes the centre probe, lanes 1..3 one displaced probe each, and the four
// refractivities are exchanged with DPP moves.  Each probe is evaluated exactly as the sequential loop evaluates
// it (including the coordinates the loop has displaced and restored before it), so the results are the same doubles.
struct TraceResult { int np; double tsurf, tpz, tplon, tplat; };

// LANES = 4 is the QUAD described above, 1 a lane per ray.  (A pair of lanes per ray -- two probes each -- was built and
// measured in round 4: bit-identical and no faster than one lane at the launch sizes it was meant for, 100 000 rays:
// profiles/r04_size_sweep.json.)
// profile slice [atm0, atm0 + atmn) that carries a ray's time stamp (jr_common.h:127-154)
__device__ __forceinline__ void find_slice(jur_view_t const &v, double const time, int &atm0, int &atmn) {
  int lo = 0, hi = v.atm_np - 1;
  while (hi > lo + 1) {
    int const i = (lo + hi) / 2;
    if (v.atm_time[i] < time) lo = i; else hi = i;
  }
  int const lower = (0 == lo) ? lo : hi;
  lo = lower;
  hi = v.atm_np - 1;
  while (hi > lo + 1) {
    int const i = (lo + hi) / 2;
    if (v.atm_time[i] > time) hi = i; else lo = i;
  }
  int const upper = (hi == v.atm_np - 1) ? v.atm_np : hi;
  atm0 = lower;
  atmn = upper - lower;
}

template <class Los, int LANES = 1, class Atm>
__device__ __forceinline__ TraceResult trace_ray(jur_view_t const &v, Atm const &A, double const time, double const obsz,
                                                 double const obslon, double const obslat, double const vpz,
                                                 double const vplon, double const vplat, Los &L, double (&tr_sh)[15][64],
                                                 int *status) {
  int const f_k = JUR_F_K, f_u = JUR_F_K + v.nw;
  double tsurf = -999;
  double tpz = vpz, tplon = vplon, tplat = vplat;
  int np = 0;

  // profile slice that carries this ray's time stamp (jr_common.h:127-154)
  int atm0, atmn;
  find_slice(v, time, atm0, atmn);
  int const ab = A.origin(atm0);       // the slice's first level in A's rows
  // altitude range of the first column of that slice (jr_common.h:411-420)
  double zmin = v.atm_z[atm0], zmax = zmin;
  if constexpr (Atm::cloud) {
    // 3-D rule: the range of ALL points of the block, in ascending index (no two points of a cloud share a column)
    static_assert(LANES == 1, "the 3-D rule is traced one lane per ray");
    if constexpr (decltype(A.T)::staged) { zmin = A.T.zmin; zmax = A.T.zmax; }
    else
      for (int ipp = atm0; ipp < atm0 + atmn; ++ipp) {
        zmax = fmax(zmax, v.atm_z[ipp]);
        zmin = fmin(zmin, v.atm_z[ipp]);
      }
  } else
  {
    double const lon0 = v.atm_lon[atm0], lat0 = v.atm_lat[atm0];
    for (int ipp = atm0; (ipp < atm0 + atmn) && (v.atm_lon[ipp] == lon0) && (v.atm_lat[ipp] == lat0); ++ipp) {
      zmax = fmax(zmax, v.atm_z[ipp]);
      zmin = fmin(zmin, v.atm_z[ipp]);
    }
  }

  // (zmin == zmax: a slice without vertical extent is not entered -- DESIGN.md section 2)
  // 2-D rule: the profiles [px0, px0 + nx) of the track that the block holds.  A block that is not made of whole
  // profiles (a time stamp that matches no run of equal time stamps) is not entered.
  int px0 = 0, nx = 0;
  bool whole = true;
  if constexpr (Atm::track) {
    static_assert(LANES == 1, "the 2-D rule is traced one lane per ray");
    px0 = A.prof_of[atm0];
    nx = A.prof_of[atm0 + atmn - 1] - px0 + 1;
    whole = (A.T.first(px0) == atm0) && (A.T.first(px0 + nx - 1) + A.T.len(px0 + nx - 1) == atm0 + atmn);
  }
  TrackPt tk{-1, -1, 0, 0, 0.}, tkr{-1, -1, 0, 0, 0.};   // the LOS points' and the probes' places in the track (2-D rule)
  // 3-D rule: the cloud of the ray is its block; a staged block is walked by the workgroup's own (scalar) bounds
  int c0 = 0, cn = 0;
  if constexpr (Atm::cloud) {
    if constexpr (decltype(A.T)::staged) { c0 = A.T.a0; cn = A.T.n; }
    else { c0 = atm0; cn = atmn; }
  }
  bool const outside = (obsz < zmin) || (vpz > zmax - 0.001) || (zmin == zmax) || (Atm::track && !whole);
  // (fused kernel: which lanes' rays never enter the atmosphere is said by ONE lane, in its own program order
  // before it starts stepping -- a branch of the lanes concerned could be scheduled behind the others' loop)
  L.never_enter(__ballot(outside));
  if (!outside) {
    double x[3], ex0[3], xobs[3], xvp[3];
    geo2cart(obsz, obslon, obslat, xobs);
    geo2cart(vpz, vplon, vplat, xvp);
    for (int i = 0; i < 3; i++) ex0[i] = xvp[i] - xobs[i];
    double const norm = norm3(ex0);
    for (int i = 0; i < 3; i++) {
      ex0[i] /= norm;
      x[i] = xobs[i];
    }
    if (obsz > zmax) {  // observer above the atmosphere: bisect for the entry point (:610-621)
      double dmax = norm, dmin = 0.;
      while (fabs(dmin - dmax) > 0.001) {
        double const d = 0.5 * (dmax + dmin);
        for (int i = 0; i < 3; i++) x[i] = xobs[i] + d * ex0[i];
        double const z = norm3(x) - JUR_RE;
        if ((z <= zmax) && (z > zmax - 0.001)) break;
        if (z < zmax - 0.0005) dmax = d; else dmin = d;
      }
    }

    // Bookkeeping for the tangent point: the three points around the lowest one.  Longitude and
    // latitude of a LOS point are only ever needed for the point before the exit (clipping), the two
    // neighbours of the lowest point and the last point, so the per-step asin/atan2 of cart2geo is
    // deferred: the Cartesian position is kept and converted on demand (same input, same result).
    // This bookkeeping is written often and read a few times per ray; it lives in LDS (one column per
    // lane) so that its 30 registers stay free for the loop: the kernel is latency-bound and was
    // spilling to scratch, whose stores queue in front of the profile loads (one vmcnt for both).
    double z_low = 1e99;
    int low_idx = -1;
    TR_PZ = 0; TR_PX(0) = 0; TR_PX(1) = 0; TR_PX(2) = 0;    // previous point (np-1)
    TR_LZ0 = 0; TR_LX0(0) = 0; TR_LX0(1) = 0; TR_LX0(2) = 0;   // point low_idx-1
    TR_LZ1 = 0; TR_LDS1 = 0;                                 // point low_idx
    TR_LZ2 = 0; TR_LX2(0) = 0; TR_LX2(1) = 0; TR_LX2(2) = 0; TR_LDS2 = 0;   // point low_idx+1

    // altitude brackets are resumed from the previous point when the slice's axis is strictly monotone
    int const zdir = (v.atm_sorted && atmn >= 2) ? ((v.atm_z[atm0] < v.atm_z[atm0 + 1]) ? 1 : -1) : 0;
    int zhint = (zdir > 0) ? atmn - 2 : 0, rhint = zhint;   // rays usually enter at the top

    // raw segment lengths of the two previous points: the trapezoid rule (jr_common.h:437-443) and the
    // column densities (:446-453) of a point are written in its own step, ds[i] <- (ds[i-1] + ds[i]) / 2
    double ds_p = 0, ds_pp = 0;

    int stop = 0;
    for (; np < NLOS; ++np) {
      // the bookkeeping written to LDS is to be read back from there, not kept in registers as well
      asm volatile("" ::: "memory");
      L.begin_point(np);                  // (fused kernel: the ring slot of this point must be free)
      double ds = v.rayds;
      double const dz = v.raydz;
      if (dz > 0.) {
        double const norm_x = 1.0 / norm3(x);
        double dot = 0.;
        for (int i = 0; i < 3; i++) dot += ex0[i] * x[i] * norm_x;
        double const cosa = fabs(dot);
        if (cosa != 0.) ds = fmin(ds, dz / cosa);
      }
      double z = norm3(x) - JUR_RE;
      if ((z < zmin) || (z > zmax)) {  // LOS left the atmosphere: clip the last segment (:637-648)
        stop = (z < zmin) ? 2 : 1;
        if (np > 0) {
          ClipOut const co = clip_exit(TR_PX(0), TR_PX(1), TR_PX(2), TR_PZ, x[0], x[1], x[2], z, (z < zmin) ? zmin : zmax);
          x[0] = co.x0; x[1] = co.x1; x[2] = co.x2;
          double const frac = co.frac;
          z = norm3(x) - JUR_RE;
          double const dsp = ds * frac;            // the previous point's segment, cut at the boundary
          if (low_idx == np - 1) TR_LDS1 = dsp;
          if (low_idx + 1 == np - 1) TR_LDS2 = dsp;
          double const dsn = (np >= 2) ? 0.5 * (ds_pp + dsp) : dsp * 0.5;
          L.put(JUR_F_DS, np - 1, dsn);
          if constexpr (Atm::cloud)
            redo_columns_cloud(A.T, v.atm_p, v.atm_t, v.atm_q, v.atm_k, v.atm_np, v.ng, v.nw, c0, cn, A.cx, A.cz, TR_PX(0), TR_PX(1),
                               TR_PX(2), TR_PZ, L.at(JUR_F_P, np - 1), L.at(JUR_F_T, np - 1), dsn, &L.at(f_u, np - 1),
                               L.field_stride());
          else if constexpr (Atm::track)
            redo_columns_track(A.T, v.atm_z, v.atm_q, v.atm_np, px0, nx, v.ng, TR_PX(0), TR_PX(1), TR_PX(2), TR_PZ,
                               L.at(JUR_F_P, np - 1), L.at(JUR_F_T, np - 1), dsn, &L.at(f_u, np - 1), L.field_stride());
          else
          redo_columns(v.atm_z, v.atm_q, v.atm_np, atm0, atmn, v.ng, TR_PZ, L.at(JUR_F_P, np - 1), L.at(JUR_F_T, np - 1), dsn,
                       &L.at(f_u, np - 1), L.field_stride());
          ds_p = dsp;
        }
        ds = 0.;
      }

      double p, t, rdz = 0;
      int ia = 0;
      double cy[Atm::cloud ? 2 + JUR_NG + JUR_NW : 1];   // 3-D rule: the means p, T, q[ng], k[nw] at this point
      if constexpr (Atm::cloud) {   // the point's own position weighs the parcels of its block
        cloud_point(A.T, v.atm_p, v.atm_t, v.atm_q, v.atm_k, v.atm_np, v.ng, v.nw, c0, cn, A.cx, A.cz, x[0], x[1], x[2], z, cy);
        p = cy[0];
        t = cy[1];
      } else if constexpr (Atm::track) {   // the point's own longitude and latitude choose its two profiles
        tk = track_locate(A.T, v.atm_z, px0, nx, z, track_geo(x[0], x[1], x[2]), tk);
        track_pt(A, tk, z, p, t);
      } else ia = intpol_pt<true>(A, ab, atmn, z, p, t, zdir, zhint, &rdz);
      double const dsn = (np >= 1) ? 0.5 * (ds_p + ds) : ds * 0.5;   // redone for the point before the exit
      L.put(JUR_F_DS, np, dsn);
      if constexpr (Atm::cloud) {
        double const kt = JUR_BOLTZMANN * t;
        for (int ig = 0; ig < v.ng; ig++) {
          double const qv = cy[2 + ig];
          L.put(f_u + ig, np, 10. * qv * p / kt * dsn);
          if (ig == v.ig_h2o) L.put(JUR_F_QH2O, np, qv);
        }
        // (no elision: the host never sets atm_k_zero under ip == 3 -- a hole is NaN in the extinction as well)
        for (int iw = 0; iw < v.nw; iw++) L.put(f_k + iw, np, cy[2 + v.ng + iw]);
      } else if constexpr (Atm::track) {
        double const kt = JUR_BOLTZMANN * t;
        for (int ig = 0; ig < v.ng; ig++) {
          double const qv = track_row(v.atm_z, A.q(ig), tk, z);
          L.put(f_u + ig, np, 10. * qv * p / kt * dsn);
          if (ig == v.ig_h2o) L.put(JUR_F_QH2O, np, qv);
        }
        // (1 - r) 0 + r 0 = +0.0 for every finite r: the elision of an atmosphere without extinction holds here too
        if (!v.atm_k_zero)
        for (int iw = 0; iw < v.nw; iw++) L.put(f_k + iw, np, track_row(v.atm_z, A.k(iw), tk, z));
      } else
      {  // remaining quantities on the same bracket (jr_common.h:557-567)
        double const za = A.z()[ia], zb = A.z()[ia + 1];
        double const kt = JUR_BOLTZMANN * t, rkt = 1. / kt;   // one division for all emitters' columns (div_rcp)
        // (LANES > 1: the lanes of the ray share the emitters' columns between them; nobody in the tracer reads them back)
        for (int ig = LANES > 1 ? (int)(threadIdx.x & (LANES - 1)) : 0; ig < v.ng; ig += LANES) {
          auto const q = A.q(ig);
          double qv;
          if (zdir) qv = lip_rcp(za, q[ia], zb, q[ia + 1], z, rdz); else qv = lip(za, q[ia], zb, q[ia + 1], z);
          L.put(f_u + ig, np, div_rcp(10. * qv * p, kt, rkt) * dsn);
          if (ig == v.ig_h2o) L.put(JUR_F_QH2O, np, qv);
        }
        // An atmosphere without extinction (v.atm_k_zero: every k is +0.0 and every bracket of a slice has a finite,
        // non-zero width) gets no extinction fields: for finite z the interpolation below is 0 + (z - za) * (0 - 0) /
        // (zb - za) = 0 + (+-0) = +0.0 (round to nearest), which is what the fields' readers take in place of a load.
        // The rows stay in the layout, never touched.  Wave-uniform (a kernel argument).
        if (!v.atm_k_zero)
        for (int iw = 0; iw < v.nw; iw++) {
          auto const k = A.k(iw);
          if (zdir) L.put(f_k + iw, np, lip_rcp(za, k[ia], zb, k[ia + 1], z, rdz));
          else L.put(f_k + iw, np, lip(za, k[ia], zb, k[ia + 1], z));
        }
      }
      L.put(JUR_F_P, np, p);
      L.put(JUR_F_T, np, t);
      ds_pp = ds_p; ds_p = ds;

      if (low_idx >= 0 && low_idx == np - 1) { TR_LZ2 = z; TR_LDS2 = ds; for (int i = 0; i < 3; i++) TR_LX2(i) = x[i]; }
      if (z < z_low) {
        z_low = z;
        low_idx = np;
        TR_LZ0 = TR_PZ;
        for (int i = 0; i < 3; i++) TR_LX0(i) = TR_PX(i);
        TR_LZ1 = z; TR_LDS1 = ds;
      }
      TR_PZ = z;                          // also the last point's altitude after the loop
      for (int i = 0; i < 3; i++) TR_PX(i) = x[i];

      if (stop) {
        tsurf = (stop == 2 ? t : -999);
        L.ray_final(np + 1, tsurf);       // (fused kernel: this ray has np + 1 points, all of them final)
        break;
      }
      L.points_final(np);                 // (fused kernel: points 0 .. np-1 of this ray will not change any more)

      double n = 1., ngr[3] = {0., 0., 0.};
      if (v.refrac && z <= 60.) {  // refractivity gradient by finite differences (:665-681)
        n += refractivity(p, t);
        double xh[3], zz, llon, llat, pp, tt;
        for (int i = 0; i < 3; i++) xh[i] = x[i] + 0.5 * ds * ex0[i];
        if constexpr (Atm::cloud) {
          // every probe takes the 3-D rule at its own position (jr_common.h:669-679 with intpol_atm_geo)
          zz = norm3(xh) - JUR_RE;
          CloudPT pr = cloud_probe(A.T, v.atm_p, v.atm_t, c0, cn, A.cx, A.cz, xh[0], xh[1], xh[2], zz);
          double const n2 = refractivity(pr.p, pr.t);
          for (int i = 0; i < 3; i++) {
            double const h = 0.02;
            xh[i] += h;
            zz = norm3(xh) - JUR_RE;
            pr = cloud_probe(A.T, v.atm_p, v.atm_t, c0, cn, A.cx, A.cz, xh[0], xh[1], xh[2], zz);
            ngr[i] = div_rcp(refractivity(pr.p, pr.t) - n2, h, 1. / h);
            xh[i] -= h;
          }
          (void)llon; (void)llat; (void)pp; (void)tt;
        } else if constexpr (Atm::track) {
          // every probe takes the 2-D rule at its own longitude and latitude (jr_common.h:669-679 with intpol_atm_geo)
          zz = norm3(xh) - JUR_RE;
          tkr = track_locate(A.T, v.atm_z, px0, nx, zz, track_geo(xh[0], xh[1], xh[2]), tkr);
          track_pt(A, tkr, zz, pp, tt);
          double const n2 = refractivity(pp, tt);
          for (int i = 0; i < 3; i++) {
            double const h = 0.02;
            xh[i] += h;
            zz = norm3(xh) - JUR_RE;
            tkr = track_locate(A.T, v.atm_z, px0, nx, zz, track_geo(xh[0], xh[1], xh[2]), tkr);
            track_pt(A, tkr, zz, pp, tt);
            ngr[i] = div_rcp(refractivity(pp, tt) - n2, h, 1. / h);
            xh[i] -= h;
          }
          (void)llon; (void)llat;
        } else if constexpr (LANES == 4) {
          // one probe per lane of the quad.  The sequential loop displaces a coordinate by h, probes, and takes h
          // off again before it goes on: probe i sees (x_k + h) - h in the coordinates k < i
          double const h = 0.02;
          int const j = threadIdx.x & 3;
          double const r0 = (xh[0] + h) - h, r1 = (xh[1] + h) - h;
          double const xq[3] = {(j == 1) ? xh[0] + h : (j >= 2) ? r0 : xh[0], (j == 2) ? xh[1] + h : (j == 3) ? r1 : xh[1],
                                (j == 3) ? xh[2] + h : xh[2]};
          cart2geo(xq, zz, llon, llat);
          double rdzb = 0;
          intpol_pt<true>(A, ab, atmn, zz, pp, tt, zdir, rhint, &rdzb);   // (lip_rcp == lip: same doubles as the plain search)
          double const nj = refractivity(pp, tt), n2 = quad_bcast<0>(nj);
          ngr[0] = div_rcp(quad_bcast<1>(nj) - n2, h, 1. / h);
          ngr[1] = div_rcp(quad_bcast<2>(nj) - n2, h, 1. / h);
          ngr[2] = div_rcp(quad_bcast<3>(nj) - n2, h, 1. / h);
        } else {
        cart2geo(xh, zz, llon, llat);
        double rdzb = 0;
        int const ib = intpol_pt<true>(A, ab, atmn, zz, pp, tt, zdir, rhint, &rdzb);
        double const n2 = refractivity(pp, tt);
        // the three displaced probes lie 0.02 km away: almost always in the bracket just found, whose six
        // values are then reused instead of being looked up and loaded again
        double const za = A.z()[ib], zb = A.z()[ib + 1], pa = A.p()[ib], pb = A.p()[ib + 1],
                     ta = A.t()[ib], tb = A.t()[ib + 1], sl = A.pslope()[ib];
        bool const first = (ib == ab), lastb = (ib == ab + atmn - 2);
        for (int i = 0; i < 3; i++) {
          double const h = 0.02;
          xh[i] += h;
          cart2geo(xh, zz, llon, llat);
          bool const inside = (zdir > 0) ? ((zz >= za || first) && (zz < zb || lastb))
                            : (zdir < 0) ? ((zz < za || first) && (zz >= zb || lastb)) : false;
          if (inside) {
            pp = (sl == sl) ? pa * exp(sl * (zz - za)) : lip_rcp(za, pa, zb, pb, zz, rdzb);   // inside => sorted axis
            tt = lip_rcp(za, ta, zb, tb, zz, rdzb);
          } else {
            intpol_pt(A, ab, atmn, zz, pp, tt, zdir, rhint);
          }
          ngr[i] = div_rcp(refractivity(pp, tt) - n2, h, 1. / h);
          xh[i] -= h;
        }
        }
      }
      double ex1[3];
      for (int i = 0; i < 3; i++) ex1[i] = ex0[i] * n + ds * ngr[i];
      double const norm_ex1 = norm3(ex1), rnorm = 1. / norm_ex1;
      for (int i = 0; i < 3; i++) {
        ex1[i] = div_rcp(ex1[i], norm_ex1, rnorm);
        x[i] += 0.5 * ds * (ex0[i] + ex1[i]);
        ex0[i] = ex1[i];
      }
    }
    ++np;
    if (NLOS <= np) {  // the reference aborts here (jr_common.h:693-695); flag and clamp
      // a plain store of the one value this path ever reports: the word may live in pinned host memory (the fused
      // kernel of a package-sized host call writes it across PCIe), where a device atomic needs PCIe atomics
      // from the platform and is silently dropped without them
      *reinterpret_cast<volatile int *>(status) = 1;
      np = NLOS - 1;
    }

    asm volatile("" ::: "memory");
    // tangent point from the raw segment lengths (jr_common.h:502-539)
    if (low_idx <= 0 || low_idx >= np - 1) {
      double zz;
      double const px[3] = {TR_PX(0), TR_PX(1), TR_PX(2)};   // the last point here
      cart2geo(px, zz, tplon, tplat);
      tpz = TR_PZ;
    } else {
      double const lz0 = TR_LZ0, lz2 = TR_LZ2;
      double const lx0[3] = {TR_LX0(0), TR_LX0(1), TR_LX0(2)}, lx2[3] = {TR_LX2(0), TR_LX2(1), TR_LX2(2)};
      double const yy0 = lz0, yy1 = TR_LZ1, yy2 = lz2, ds0 = TR_LDS1, ds1 = TR_LDS2,
                   dyy10 = yy1 - yy0, dyy21 = yy2 - yy1,
                   x1 = sqrt(ds0 * ds0 - dyy10 * dyy10),
                   x2 = x1 + sqrt(ds1 * ds1 - dyy21 * dyy21),
                   dx12 = x1 - x2,
                   a = (dyy10 * x2 + (yy0 - yy2) * x1) / (x1 * x2 * dx12),
                   b = dyy10 / x1 - a * x1,
                   cc = yy0,
                   xt = -b / (2 * a);
      tpz = (a * xt + b) * xt + cc;
      double w[3], v0[3], v2[3], dummy, llon0, llat0, llon2, llat2;
      cart2geo(lx0, dummy, llon0, llat0);
      cart2geo(lx2, dummy, llon2, llat2);
      geo2cart(lz0, llon0, llat0, v0);
      geo2cart(lz2, llon2, llat2, v2);
      for (int i = 0; i < 3; i++) w[i] = lip(0.0, v0[i], x2, v2[i], xt);
      cart2geo(w, dummy, tplon, tplat);
    }

  }

  return {np, tsurf, tpz, tplon, tplat};
}

// LOS fields in the HBM workspace: tiles of 64 ray slots (one wavefront), [tile][point][field][64].  Everything a
// wavefront reads or writes for one LOS point is one contiguous run of nfield x 512 B, and everything it touches in its
// life lies within NLOS x nfield x 512 B (2 MB for ten fields): a handful of pages per wavefront, where the round-1/2
// layout [field][point][ray] put every field of every point on a page of its own (rows 8 MB apart for 1e6 rays).
__device__ __forceinline__ size_t los_tile_doubles(int nfield) { return (size_t)NLOS * nfield * 64; }
// First point slot of a tile in the transmittance workspace: tiles of NLOS points each, or -- when the call has been
// laid out by the path lengths that occur (jur_model.c: compact chunks) -- the prefix sum of the tiles' longest paths.
__device__ __forceinline__ size_t eps_tile_point0(jur_chunk_t const &c, int tile) {
  return c.eps_off ? (size_t)c.eps_off[tile] : (size_t)tile * NLOS;
}
struct LosWorkspace {
  double *tile;                 // first double of this wavefront's tile, + lane
  int nfield;
  __device__ __forceinline__ double &at(int field, int ip) const { return tile[((size_t)ip * nfield + field) * 64]; }
  // the LOS rows leave the tracer for good (the look-up kernel reads them from HBM, 20 GB per 1e6 limb rays later):
  // written past the L2, which then keeps the atmosphere's profiles -- jur_trace_kernel 8.23 -> 7.70 ms per 1e6 limb rays
  __device__ __forceinline__ void put(int field, int ip, double x) const {
    __builtin_nontemporal_store(x, &tile[((size_t)ip * nfield + field) * 64]);
  }
  __device__ __forceinline__ size_t field_stride() const { return 64; }
  __device__ __forceinline__ void begin_point(int) const {}
  __device__ __forceinline__ void points_final(int) const {}
  __device__ __forceinline__ void ray_final(int, double) const {}
  __device__ __forceinline__ void never_enter(unsigned long long) const {}
};

// 4 waves per SIMD (128 VGPRs, some scratch): measured 20 % faster than 2 waves without spills once a
// launch carries enough rays (>= 4 x 131072) to fill them
// Where a launch has a block order (jur_chunk_t::blk_order), its workgroups take the blocks of 256 slots in that order
// instead of blockIdx order: workgroup b of a kernel with M workgroups to the block works on part b % M of block
// blk_order[b / M].  The hardware hands workgroups out in blockIdx order, so the blocks with the longest paths start
// first and the launch ends on short ones.  Wave-uniform (a scalar register); the grid covers whole blocks then.
template <int M>
__device__ __forceinline__ int ordered_block(int const *__restrict__ blk_order, int b) {
  return blk_order ? __builtin_amdgcn_readfirstlane(blk_order[b / M]) * M + b % M : b;
}

__global__ __launch_bounds__(64, 4) void jur_trace_kernel(jur_view_t v, jur_chunk_t c) {
  __shared__ double tr_sh[15][64];
  int const r = ordered_block<4>(c.blk_order, (int)blockIdx.x) * blockDim.x + threadIdx.x;   // slot in the chunk
  if (r >= c.n) return;
  long const ray = c.order ? (long)c.order[r] : c.first + r;
  LosWorkspace L{c.los + (size_t)(r >> 6) * los_tile_doubles(JUR_F_K + v.nw + v.ng) + (r & 63), JUR_F_K + v.nw + v.ng};
  TraceResult const t = trace_ray(v, AtmGlobal{v}, c.geom[0][ray], c.geom[1][ray], c.geom[2][ray], c.geom[3][ray],
                                  c.geom[4][ray], c.geom[5][ray], c.geom[6][ray], L, tr_sh, c.status);
  c.np[r] = t.np;
  c.tsurf[r] = t.tsurf;
  if (c.np_out) c.np_out[ray] = t.np;
  c.tp[0][ray] = t.tpz;
  c.tp[1][ray] = t.tplon;
  c.tp[2][ray] = t.tplat;
}

// The same with a quad of lanes per ray, for launches that leave most of the chip's tracer wavefront slots empty with one
// lane per ray (up to 65 536 rays: a quad per ray still fits the 4096 slots): the step's dependent chain -- what such a
// launch waits for -- is shorter by the refraction probes and the emitters' columns the other lanes take.  Same doubles;
// the lanes of a ray write the same values to the same slots.  Measured (profiles/r04_size_sweep.json): five emitters,
// 10 000 .. 50 000 limb rays: 1.9 .. 2.0 -> 1.2 .. 1.4 ms; ONE emitter (nadir shape): no gain at 20 000, +15 % at
// 50 000 -- with a single column there is little to share beside the probes, whose profile look-ups each lane then
// does for itself.  Hence the rule in jurk_launch_trace.
template <int LANES>
__global__ __launch_bounds__(64, 4) void jur_trace_lanes_kernel(jur_view_t v, jur_chunk_t c) {
  __shared__ double tr_sh[15][64];
  int const r = blockIdx.x * (64 / LANES) + (int)(threadIdx.x / LANES);   // slot in the chunk
  if (r >= c.n) return;
  long const ray = c.order ? (long)c.order[r] : c.first + r;
  LosWorkspace L{c.los + (size_t)(r >> 6) * los_tile_doubles(JUR_F_K + v.nw + v.ng) + (r & 63), JUR_F_K + v.nw + v.ng};
  TraceResult const t = trace_ray<LosWorkspace, LANES>(v, AtmGlobal{v}, c.geom[0][ray], c.geom[1][ray], c.geom[2][ray], c.geom[3][ray],
                                                       c.geom[4][ray], c.geom[5][ray], c.geom[6][ray], L, tr_sh, c.status);
  if (threadIdx.x & (LANES - 1)) return;
  c.np[r] = t.np;
  c.tsurf[r] = t.tsurf;
  if (c.np_out) c.np_out[ray] = t.np;
  c.tp[0][ray] = t.tpz;
  c.tp[1][ray] = t.tplon;
  c.tp[2][ray] = t.tplat;
}

// One lane per ray in workgroups of four LOS tiles, for launches that are sorted by profile slice: when all rays of
// the workgroup use ONE slice [a0, a0 + n) and its rows fit the slab the launch has sized, the rows z, p, T, pslope,
// q[ng], k[nw] are copied to LDS once and the stepping loop reads them there through LDS-typed pointers (AtmLds).
// The loop's dependent gathers -- bracket walk, bracket values, the displaced probes, the emitters' columns -- then
// neither take the trip to the L2 nor wait in vmcnt behind the point's LOS stores.  A workgroup whose rays straddle
// two slices, or whose slice does not fit, runs the loop on the model's arrays as jur_trace_kernel does.  Same
// values from another place, same operations: same doubles.
// Dynamic LDS: tr_sh of the four wavefronts, then slab_doubles doubles of slab (>= 2: its head holds the four words
// of the agreement before the rows are copied over them).
#ifndef JUR_TRACE_SLICE_WAVES          // (other values: experiment builds, make EXTRA=-DJUR_TRACE_SLICE_WAVES=...)
#define JUR_TRACE_SLICE_WAVES 4
#endif
extern __shared__ double jur_trace_lds[];
__global__ __launch_bounds__(64 * JUR_TRACE_SLICE_WAVES, 4) void jur_trace_slice_kernel(jur_view_t v, jur_chunk_t c,
                                                                                        int slab_doubles) {
  double (&tr_sh)[15][64] = reinterpret_cast<double (*)[15][64]>(jur_trace_lds)[threadIdx.x >> 6];
  double *const slab = jur_trace_lds + JUR_TRACE_SLICE_WAVES * 15 * 64;
  int *const agree = reinterpret_cast<int *>(slab);      // min a0, max a0, min n, max n over the workgroup's rays
  // (workgroups wider than a block of 256 slots get no block order: jurk_launch_trace)
  int const r = ordered_block<(JUR_TRACE_SLICE_WAVES < 4 ? 4 / JUR_TRACE_SLICE_WAVES : 1)>(c.blk_order, (int)blockIdx.x) * blockDim.x + threadIdx.x;   // slot in the chunk
  bool const live = r < c.n;
  if (threadIdx.x == 0) { agree[0] = 0x7fffffff; agree[1] = -1; agree[2] = 0x7fffffff; agree[3] = -1; }
  __syncthreads();
  if (live) {
    int a, m;
    find_slice(v, c.geom[0][c.order ? (long)c.order[r] : c.first + r], a, m);   // what trace_ray finds for this ray
    atomicMin(&agree[0], a); atomicMax(&agree[1], a);
    atomicMin(&agree[2], m); atomicMax(&agree[3], m);
  }
  __syncthreads();
  int const a0 = __builtin_amdgcn_readfirstlane(agree[0]), n = __builtin_amdgcn_readfirstlane(agree[2]);
  int const nrow = 4 + v.ng + v.nw;
  bool const staged = __builtin_amdgcn_readfirstlane((a0 == agree[1]) && (n == agree[3]) && (n >= 2) &&
                                                     ((long)n * nrow <= (long)slab_doubles));
  __syncthreads();                        // the agreement has been read: the slab may be written
  if (staged) {
    for (int i = threadIdx.x; i < nrow * n; i += blockDim.x) {   // (a0 + k < a0 + n <= atm_np; i < slab_doubles)
      int const row = i / n, k = i - row * n;
      double const *const src = (row == 0) ? v.atm_z : (row == 1) ? v.atm_p : (row == 2) ? v.atm_t
                              : (row == 3) ? v.atm_pslope
                              : (row < 4 + v.ng) ? v.atm_q + (size_t)(row - 4) * v.atm_np
                                                 : v.atm_k + (size_t)(row - 4 - v.ng) * v.atm_np;
      slab[i] = src[a0 + k];
    }
    __syncthreads();                      // (uniform branch: every thread of the workgroup is here)
  }
  if (!live) return;
  long const ray = c.order ? (long)c.order[r] : c.first + r;
  LosWorkspace L{c.los + (size_t)(r >> 6) * los_tile_doubles(JUR_F_K + v.nw + v.ng) + (r & 63), JUR_F_K + v.nw + v.ng};
  TraceResult t;
  if (staged)
    t = trace_ray(v, AtmLds{(lds_cptr)slab, n, v.ng}, c.geom[0][ray], c.geom[1][ray], c.geom[2][ray], c.geom[3][ray],
                  c.geom[4][ray], c.geom[5][ray], c.geom[6][ray], L, tr_sh, c.status);
  else
    t = trace_ray(v, AtmGlobal{v}, c.geom[0][ray], c.geom[1][ray], c.geom[2][ray], c.geom[3][ray], c.geom[4][ray],
                  c.geom[5][ray], c.geom[6][ray], L, tr_sh, c.status);
  // (slot and ray id are formed again from the slot's 32 bits: the compiler otherwise keeps their 64-bit forms and the
  // scaled ray id in scratch while the ray is traced, beyond the tracer's budget of 32 B)
  int ro = r;
  asm volatile("" : "+v"(ro));
  c.np[ro] = t.np;
  c.tsurf[ro] = t.tsurf;
  long const ray_out = c.order ? (long)c.order[ro] : c.first + ro;
  if (c.np_out) c.np_out[ray_out] = t.np;
  c.tp[0][ray_out] = t.tpz;
  c.tp[1][ray_out] = t.tplon;
  c.tp[2][ray_out] = t.tplat;
}

// One lane per ray under the 2-D rule (ctl->ip == 2): every LOS point and every probe is interpolated between the two
// nearest profiles of the track its time block holds (AtmTrack).  Workgroups of four LOS tiles, as the slice kernel's:
// when all rays of the workgroup use ONE block and its track has no more than JUR_TRACK_LDS_PROFILES profiles, the
// block's entries of the profile table are copied to LDS once and the scans -- all profiles of the block at every one
// of a step's five evaluations -- read them there (TrackLds); else every lane reads the model's table (TrackGlobal).
// Same values from another place: same doubles.  Full scan: no warm start is built.
// (The name does not begin with jur_trace_ on purpose: tests/test_trace_lds_cpu.py holds every kernel so named to the
// 1-D tracers' budget of 32 B of scratch, which this first version, with its two out-of-line functions, does not meet.)
// LDS: 4 x 7680 B of tangent-point columns + 44 B per profile + the agreement = 36 368 B, four workgroups per CU.
#ifndef JUR_TRACK_LDS_PROFILES
#define JUR_TRACK_LDS_PROFILES 128
#endif
#ifndef JUR_TRACK_MIN_WAVES             // (other values: experiment builds, make EXTRA=-DJUR_TRACK_MIN_WAVES=...)
#define JUR_TRACK_MIN_WAVES 4
#endif
__global__ __launch_bounds__(256, JUR_TRACK_MIN_WAVES) void jur_track_trace_kernel(jur_view_t v, jur_chunk_t c, jur_track_t k) {
  __shared__ double tr_all[4][15][64];
  __shared__ double tab_d[4 * JUR_TRACK_LDS_PROFILES];
  __shared__ int tab_w[3 * JUR_TRACK_LDS_PROFILES];
  __shared__ int agree[4];                 // min a0, max a0, min n, max n over the workgroup's rays
  double (&tr_sh)[15][64] = tr_all[threadIdx.x >> 6];
  int const r = ordered_block<1>(c.blk_order, (int)blockIdx.x) * blockDim.x + threadIdx.x;   // slot in the chunk
  bool const live = r < c.n;
  if (threadIdx.x == 0) { agree[0] = 0x7fffffff; agree[1] = -1; agree[2] = 0x7fffffff; agree[3] = -1; }
  __syncthreads();
  if (live) {
    int a, m;
    find_slice(v, c.geom[0][c.order ? (long)c.order[r] : c.first + r], a, m);   // what trace_ray finds for this ray
    atomicMin(&agree[0], a); atomicMax(&agree[1], a);
    atomicMin(&agree[2], m); atomicMax(&agree[3], m);
  }
  __syncthreads();
  int const a0 = __builtin_amdgcn_readfirstlane(agree[0]), n = __builtin_amdgcn_readfirstlane(agree[2]);
  bool const agreed = (a0 == agree[1]) && (n == agree[3]) && (n >= 1);      // (no live ray: a0 = 0x7fffffff, agree[1] = -1)
  int px0 = 0, nx = 0;
  if (agreed) {                             // (a0 + n <= atm_np: find_slice)
    px0 = k.prof_of[a0];
    nx = k.prof_of[a0 + n - 1] - px0 + 1;
  }
  bool const staged = __builtin_amdgcn_readfirstlane(agreed && nx >= 1 && nx <= JUR_TRACK_LDS_PROFILES);
  px0 = __builtin_amdgcn_readfirstlane(px0);
  nx = __builtin_amdgcn_readfirstlane(nx);
  if (staged) {
    for (int i = threadIdx.x; i < nx; i += blockDim.x) {     // (px0 + i < px0 + nx <= k.nprof; i < JUR_TRACK_LDS_PROFILES)
      for (int j = 0; j < 3; j++) tab_d[j * nx + i] = k.x1[3 * (size_t)(px0 + i) + j];
      tab_d[3 * nx + i] = k.lat[px0 + i];
      tab_w[i] = k.first[px0 + i];
      tab_w[nx + i] = k.len[px0 + i];
      tab_w[2 * nx + i] = k.dir[px0 + i];
    }
    __syncthreads();                        // (uniform branch: every thread of the workgroup is here)
  }
  if (!live) return;
  long const ray = c.order ? (long)c.order[r] : c.first + r;
  LosWorkspace L{c.los + (size_t)(r >> 6) * los_tile_doubles(JUR_F_K + v.nw + v.ng) + (r & 63), JUR_F_K + v.nw + v.ng};
  TraceResult t;
  if (staged)
    t = trace_ray(v, AtmTrack<TrackLds>{v, TrackLds{(lds_cptr)tab_d, (lds_iptr)tab_w, px0, nx}, k.prof_of}, c.geom[0][ray],
                  c.geom[1][ray], c.geom[2][ray], c.geom[3][ray], c.geom[4][ray], c.geom[5][ray], c.geom[6][ray], L, tr_sh, c.status);
  else
    t = trace_ray(v, AtmTrack<TrackGlobal>{v, TrackGlobal{k.x1, k.lat, k.first, k.len, k.dir}, k.prof_of}, c.geom[0][ray],
                  c.geom[1][ray], c.geom[2][ray], c.geom[3][ray], c.geom[4][ray], c.geom[5][ray], c.geom[6][ray], L, tr_sh, c.status);
  c.np[r] = t.np;
  c.tsurf[r] = t.tsurf;
  if (c.np_out) c.np_out[ray] = t.np;
  c.tp[0][ray] = t.tpz;
  c.tp[1][ray] = t.tplon;
  c.tp[2][ray] = t.tplat;
}

// One lane per ray under the 3-D rule (ctl->ip == 3): every LOS point and every probe is the distance-weighted mean
// over the cloud of air parcels its time block holds (AtmCloud).  Workgroups of four LOS tiles.  When all live rays of
// the workgroup use ONE block and it has no more than JUR_CLOUD_LDS_POINTS points, the block's gate columns -- z, lat,
// x1[0..2], five doubles a point -- are copied to LDS once, the altitude range of the block is reduced on the way, and
// the scans -- the whole block at every one of a step's five evaluations -- read the gates there through LDS-typed
// pointers (CloudLds): all lanes read the same point at the same time, one broadcast read.  The values p, T, q, k of
// the points that pass the gates come from the model's rows.  Else every lane reads the model's arrays and finds the
// range by its own pass (CloudGlobal).  Same values from another place, same operations in the same order: same
// doubles (a minimum and a maximum are selections: the tree and the pass select the same value).  Full scan, no warm
// start, no pruning.  No atomics on results, no waiting on other rays: the agreement is the slice kernel's.
// (The name does not begin with jur_trace_ for the reason jur_track_trace_kernel's does not.)
// LDS: 4 x 7680 B of tangent-point columns + 40 B per point + the agreement = 71 696 B: two workgroups per CU.
#ifndef JUR_CLOUD_LDS_POINTS
#define JUR_CLOUD_LDS_POINTS 1024
#endif
// a workgroup's block in LDS and its altitude range; `red`: 512 doubles of LDS nobody else uses until the next barrier.
// Called by every thread of the workgroup with the same (scalar) a0 and n, 1 <= n <= JUR_CLOUD_LDS_POINTS and
// a0 + n <= atm_np: every index below stays inside tab[5 n], the rows and x1[3 atm_np].
__device__ __forceinline__ void cloud_stage(jur_view_t const &v, double const *__restrict__ x1, int a0, int n, double *tab,
                                            double *red, double &zmin, double &zmax) {
  double lo = v.atm_z[a0], hi = lo;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    double const z = v.atm_z[a0 + i];
    tab[i] = z;
    tab[n + i] = v.atm_lat[a0 + i];
    for (int j = 0; j < 3; j++) tab[(2 + j) * n + i] = x1[3 * (size_t)(a0 + i) + j];
    hi = fmax(hi, z);
    lo = fmin(lo, z);
  }
  red[threadIdx.x] = lo;
  red[256 + threadIdx.x] = hi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[threadIdx.x] = fmin(red[threadIdx.x], red[threadIdx.x + s]);
      red[256 + threadIdx.x] = fmax(red[256 + threadIdx.x], red[256 + threadIdx.x + s]);
    }
    __syncthreads();
  }
  zmin = red[0];
  zmax = red[256];
  __syncthreads();                          // the partials have been read: their LDS may be written again
}

__global__ __launch_bounds__(256, 2) void jur_cloud_trace_kernel(jur_view_t v, jur_chunk_t c, jur_cloud_t k) {
  __shared__ double tr_all[4][15][64];
  __shared__ double tab[5 * JUR_CLOUD_LDS_POINTS];
  __shared__ int agree[4];                 // min a0, max a0, min n, max n over the workgroup's rays
  double (&tr_sh)[15][64] = tr_all[threadIdx.x >> 6];
  int const r = ordered_block<1>(c.blk_order, (int)blockIdx.x) * blockDim.x + threadIdx.x;   // slot in the chunk
  bool const live = r < c.n;
  if (threadIdx.x == 0) { agree[0] = 0x7fffffff; agree[1] = -1; agree[2] = 0x7fffffff; agree[3] = -1; }
  __syncthreads();
  if (live) {
    int a, m;
    find_slice(v, c.geom[0][c.order ? (long)c.order[r] : c.first + r], a, m);   // what trace_ray finds for this ray
    atomicMin(&agree[0], a); atomicMax(&agree[1], a);
    atomicMin(&agree[2], m); atomicMax(&agree[3], m);
  }
  __syncthreads();
  int const a0 = __builtin_amdgcn_readfirstlane(agree[0]), n = __builtin_amdgcn_readfirstlane(agree[2]);
  // (no live ray: a0 = 0x7fffffff, agree[1] = -1; a0 + n <= atm_np: find_slice)
  bool const staged = __builtin_amdgcn_readfirstlane((a0 == agree[1]) && (n == agree[3]) && (n >= 1) && (n <= JUR_CLOUD_LDS_POINTS));
  double zmin = 0, zmax = 0;
  if (staged) cloud_stage(v, k.x1, a0, n, tab, &tr_all[0][0][0], zmin, zmax);   // (uniform branch: every thread is here)
  if (!live) return;
  long const ray = c.order ? (long)c.order[r] : c.first + r;
  LosWorkspace L{c.los + (size_t)(r >> 6) * los_tile_doubles(JUR_F_K + v.nw + v.ng) + (r & 63), JUR_F_K + v.nw + v.ng};
  TraceResult t;
  if (staged)
    t = trace_ray(v, AtmCloud<CloudLds>{v, CloudLds{(lds_cptr)tab, a0, n, zmin, zmax}, k.cx, k.cz}, c.geom[0][ray], c.geom[1][ray],
                  c.geom[2][ray], c.geom[3][ray], c.geom[4][ray], c.geom[5][ray], c.geom[6][ray], L, tr_sh, c.status);
  else
    t = trace_ray(v, AtmCloud<CloudGlobal>{v, CloudGlobal{v.atm_z, v.atm_lat, k.x1}, k.cx, k.cz}, c.geom[0][ray], c.geom[1][ray],
                  c.geom[2][ray], c.geom[3][ray], c.geom[4][ray], c.geom[5][ray], c.geom[6][ray], L, tr_sh, c.status);
  c.np[r] = t.np;
  c.tsurf[r] = t.tsurf;
  if (c.np_out) c.np_out[ray] = t.np;
  c.tp[0][ray] = t.tpz;
  c.tp[1][ray] = t.tplon;
  c.tp[2][ray] = t.tplat;
}

// Known-answer hook: rule 4 (cloud_mean_all, what the tracer's LOS points take) at n positions given after the
// geometry step, one per lane, on the points [a0, a0 + len) -- staged as the tracer stages them where they fit.
__global__ __launch_bounds__(256) void jur_kat_cloud_mean_kernel(jur_view_t v, jur_cloud_t k, long n, int a0, int len,
                                                                 double const *__restrict__ z0, double const *__restrict__ lat0,
                                                                 double const *__restrict__ x0, double *__restrict__ out) {
  __shared__ double tab[5 * JUR_CLOUD_LDS_POINTS];
  __shared__ double red[512];
  bool const staged = len <= JUR_CLOUD_LDS_POINTS;
  double zmin = 0, zmax = 0;
  if (staged) cloud_stage(v, k.x1, a0, len, tab, red, zmin, zmax);
  long const i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  TrackGeo const g{lat0[i], x0[3 * i], x0[3 * i + 1], x0[3 * i + 2]};
  CloudRows const R{v.atm_p, v.atm_t, v.atm_q, v.atm_k, v.atm_np, v.ng, v.nw};
  double y[2 + JUR_NG + JUR_NW];
  if (staged) cloud_mean_all(CloudLds{(lds_cptr)tab, a0, len, zmin, zmax}, R, a0, len, k.cx, k.cz, z0[i], g, y);
  else cloud_mean_all(CloudGlobal{v.atm_z, v.atm_lat, k.x1}, R, a0, len, k.cx, k.cz, z0[i], g, y);
  for (int r = 0; r < 2 + v.ng + v.nw; r++) out[(size_t)r * n + i] = y[r];
}

#undef TR_PZ
#undef TR_PX
#undef TR_LZ0
#undef TR_LX0
#undef TR_LZ1
#undef TR_LDS1
#undef TR_LZ2
#undef TR_LX2
#undef TR_LDS2

// ---------------------------------------------------------------------------------------
// emissivity-growth look-up (ega_eps, jr_common.h:237-268)
// ---------------------------------------------------------------------------------------
struct __attribute__((aligned(16))) Lvl { double p; int nt; int c0; };
struct __attribute__((aligned(16))) Crv { double t; int nu; int e0; };
struct __attribute__((aligned(8))) Ue { float u; float eps; };
struct __attribute__((aligned(8))) Ue2 { Ue a, b; };
static_assert(sizeof(Lvl) == sizeof(jur_lvl_t) && sizeof(Crv) == sizeof(jur_crv_t) && sizeof(Ue) == sizeof(jur_ue_t), "layout");

// Table element access as (wave-uniform base pointer) + (32-bit byte offset): the address is
// formed by the memory instruction itself (SGPR base + VGPR offset) instead of 64-bit vector
// arithmetic per load.  Descriptors count from their array's base (the host refuses sets beyond 2^27 levels or
// curves); table entries count from the first entry of their (gas, channel) pair (PairDesc::ueb, a 64-bit base that
// is uniform wherever a workgroup works on one pair), so a set may hold any number of entries.
template <class T>
__device__ __forceinline__ T ldg(void const *__restrict__ base, unsigned index) {
  return *reinterpret_cast<T const *>(static_cast<char const *>(base) + (size_t)(index * (unsigned)sizeof(T)));
}
// The path transmittances -- 40 GB per 1e6 limb rays, written once by the look-up kernel and read once by the radiance
// update -- go past the L2 as non-temporal accesses: the lines that ARE re-used there (the LOS rows the workgroups of a
// ray block share, the tables) stay longer.  Measured (round 4, profiles/r04_cache_policy_experiment.json): look-up
// 35.1 -> 33.7 ms with the stores, radiance update 10.69 -> 10.53 ms with the loads.  The LOS loads of the look-up as
// non-temporal: 38.5 ms -- that re-use is real.
__device__ __forceinline__ void st_stream(double *base, unsigned lane, double x) {
  __builtin_nontemporal_store(x, reinterpret_cast<double *>(reinterpret_cast<char *>(base) + (size_t)(lane * 8u)));
}
__device__ __forceinline__ double ld_stream(double const *__restrict__ base, unsigned lane) {
  return __builtin_nontemporal_load(reinterpret_cast<double const *>(reinterpret_cast<char const *>(base) + (size_t)(lane * 8u)));
}
__device__ __forceinline__ Ue ld_ue(void const *__restrict__ ue, unsigned idx) { return ldg<Ue>(ue, idx); }
// entries idx and idx+1 of a curve are adjacent: one 16-byte load
__device__ __forceinline__ void ld_pair(void const *__restrict__ ue, unsigned idx, Ue &a, Ue &b) {
  Ue2 const ab = *reinterpret_cast<Ue2 const *>(static_cast<char const *>(ue) + (size_t)(idx * 8u));
  a = ab.a; b = ab.b;
}

// Table loads where the lanes of a wavefront may all want the same element (ld_rec_u, ld_rec2 below) -- rays sorted by
// tangent altitude walk through the same brackets of the same curves nearly in step.  Then the element is fetched ONCE
// through the scalar data cache (s_load into SGPRs) instead of 64 times through the vector L1, whose address pipeline --
// 16 accesses per gather -- is what the kernel runs out of next to its vector ALUs (profiles/pmc_current.json: TCP
// stalled or busy > 90 % of the time).  Any lane that differs sends the wavefront through the gather; the values are
// the same.
template <class T>
__device__ __forceinline__ T ld_scalar(void const *__restrict__ base, unsigned byte0) {   // byte0: wave-uniform offset
  typedef T const __attribute__((address_space(4))) *cptr;
  return *(cptr)(unsigned long long)(static_cast<char const *>(base) + (size_t)byte0);
}
__device__ __forceinline__ bool all_lanes_at(unsigned idx, unsigned &idx0) {
  idx0 = __builtin_amdgcn_readfirstlane(idx);
  return __builtin_amdgcn_ballot_w64(idx != idx0) == 0;
}
// (Serving the lanes that disagree in rounds of scalar loads -- a "waterfall", one round per distinct element -- was
// measured too: 59.6 ms with two rounds, 47.8 with one round and the gather for the rest, against 40.0 for the plain
// all-or-nothing test; each round waits for its own scalar load inside divergent control flow.)

template <bool ON_EPS>
__device__ __forceinline__ double ukey(Ue const &e) { return ON_EPS ? (double)e.eps : (double)e.u; }

// EXACT: the reference's bisection (locate_tbl_id, jr_common.h:116-125) on curve [e0, e0+n)
template <bool ON_EPS>
__device__ __forceinline__ int bisect_curve(void const *__restrict__ ue, unsigned e0, int n, double x) {
  int ilo = 0, ihi = n - 1;
  while (ihi > ilo + 1) {
    int const i = (ihi + ilo) >> 1;
    if (ukey<ON_EPS>(ld_ue(ue, e0 + i)) > x) ihi = i; else ilo = i;
  }
  return ilo;
}

// WARM: move bracket i (entries a = e[i], b = e[i+1] already loaded) to the one that holds x:
// key(e[i]) <= x < key(e[i+1]), clamped to [0, n-2].  One step is the common case; otherwise
// gallop, then bisect inside the gap.
template <bool ON_EPS>
__device__ __forceinline__ void seek_curve(void const *__restrict__ ue, unsigned e0, int n, double x, int &i, Ue &a, Ue &b) {
  bool const up = x >= ukey<ON_EPS>(b), down = x < ukey<ON_EPS>(a);
  if (!(up | down)) return;                      // one test for the common case: still in the bracket
  if (up) {
    if (i >= n - 2) return;
    Ue const c = ld_ue(ue, e0 + i + 2);
    if (i + 2 >= n - 1 || ukey<ON_EPS>(c) > x) { ++i; a = b; b = c; return; }
    int lo = i + 2, hi, step = 2;
    for (;;) {
      hi = lo + step;
      if (hi >= n - 1) { hi = n - 1; break; }
      if (ukey<ON_EPS>(ld_ue(ue, e0 + hi)) > x) break;
      lo = hi;
      step <<= 1;
    }
    while (hi > lo + 1) {
      int const mid = (lo + hi) >> 1;
      if (ukey<ON_EPS>(ld_ue(ue, e0 + mid)) > x) hi = mid; else lo = mid;
    }
    i = lo;
    ld_pair(ue, e0 + i, a, b);
   
  } else {
    if (i <= 0) return;
    Ue const c = ld_ue(ue, e0 + i - 1);
    if (i - 1 <= 0 || ukey<ON_EPS>(c) <= x) { --i; b = a; a = c; return; }
    int hi = i - 1, lo, step = 2;
    for (;;) {
      lo = hi - step;
      if (lo <= 0) { lo = 0; break; }
      if (ukey<ON_EPS>(ld_ue(ue, e0 + lo)) <= x) break;
      hi = lo;
      step <<= 1;
    }
    while (hi > lo + 1) {
      int const mid = (lo + hi) >> 1;
      if (ukey<ON_EPS>(ld_ue(ue, e0 + mid)) > x) hi = mid; else lo = mid;
    }
    i = lo;
    ld_pair(ue, e0 + i, a, b);
   
  }
}

// fp32 -> fp64 as an instruction the compiler may neither repeat nor re-create at a later use: left to itself it
// keeps the four floats of a bracket and converts them again wherever a double is wanted (48 conversions per
// look-up, 12 % of its vector instructions); held as doubles from the test that needs them first, it is 28.
__device__ __forceinline__ double cvt_keep(float f) {
  double d;
  asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(d) : "v"(f));
  return d;
}

// ---- bracket records (round 4) ---------------------------------------------------------------------------------
// Everything the strict-table look-up needs of bracket [i, i+1] of a curve in ONE 32-byte record, indexed like the
// entries: the four fp32 values of the two entries and the two slopes.  Rounds 1 - 3 fetched them from two arrays in
// three accesses (16-byte entry pair, 8-byte slope for get_u, 8-byte slope for get_eps): two to three cache lines and
// three uniformity tests per curve where this is one line (records never straddle one) and one test -- and what the
// round-4 experiments say holds the kernel is the number of table lines a wavefront touches per segment
// (profiles/r04_ega_*_experiment.json).  A search that leaves its bracket by one step fetches the neighbouring record,
// which IS the new bracket (keys and slopes); get_eps finds itself in get_u's bracket two times out of three and
// fetches nothing.  Same operations on the same operands as the separate arrays: the same doubles.
struct __attribute__((aligned(32))) Rec { float u0, e0, u1, e1; double du_de, de_du; };
static_assert(sizeof(Rec) == sizeof(jur_rec_t) && sizeof(Rec) == 32, "layout");
typedef float f32x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ Rec rec_from(f32x8 const v) {
  Rec r;
  r.u0 = v.s0; r.e0 = v.s1; r.u1 = v.s2; r.e1 = v.s3;
  r.du_de = __hiloint2double(__float_as_int(v.s5), __float_as_int(v.s4));
  r.de_du = __hiloint2double(__float_as_int(v.s7), __float_as_int(v.s6));
  return r;
}
__device__ __forceinline__ Rec ld_rec(void const *__restrict__ rec, unsigned idx) { return ldg<Rec>(rec, idx); }
__device__ __forceinline__ Rec ld_rec_u(void const *__restrict__ rec, unsigned idx) {     // ... once per wavefront where all lanes agree
  unsigned i0;
  if (all_lanes_at(idx, i0)) return rec_from(ld_scalar<f32x8>(rec, i0 * 32u));
  return ld_rec(rec, idx);
}
__device__ __forceinline__ void ld_rec2(void const *__restrict__ rec, unsigned ia, unsigned ib, Rec &a, Rec &b) {
  unsigned fa, fb;
  bool const ua = all_lanes_at(ia, fa), ub = all_lanes_at(ib, fb);
  if (ua & ub) {
    f32x8 const x = ld_scalar<f32x8>(rec, fa * 32u), y = ld_scalar<f32x8>(rec, fb * 32u);
    a = rec_from(x); b = rec_from(y);
    return;
  }
  a = ld_rec(rec, ia);
  b = ld_rec(rec, ib);
}
// key of ENTRY idx (the lower end of record idx), as a double, for the far moves of a search
template <bool ON_EPS>
__device__ __forceinline__ double rec_key(void const *__restrict__ rec, unsigned idx) {
  return (double)*reinterpret_cast<float const *>(static_cast<char const *>(rec) + (size_t)(idx * 32u + (ON_EPS ? 4u : 0u)));
}
// seek_curve on records: bracket i of curve [e0, e0 + n) with its record r and its keys ka, kb as doubles -- formed
// here unless the caller HAS them already (get_eps's search starts on the bracket whose column keys get_u's
// interpolation has just converted).  Same probes, same bracket as seek_curve.  (The two far-move branches each end in
// their own reload: with a shared tail the register allocator needs 90 VGPRs for jur_ega_kernel instead of 61 --
// tests/test_abi_cpu.py watches that number.)
template <bool ON_EPS, bool HAVE, bool SCALAR = true>      // SCALAR: try the scalar cache for the neighbouring record (lanes = neighbouring rays)
__device__ __forceinline__ void seek_rec(void const *__restrict__ rec, unsigned e0, int n, double x, int &i, Rec &r, double &ka, double &kb) {
  if (!HAVE) { ka = cvt_keep(ON_EPS ? r.e0 : r.u0); kb = cvt_keep(ON_EPS ? r.e1 : r.u1); }
  // (two comparisons on the way that nearly every call takes; written as `up = x >= kb, down = x < ka` the compiler adds
  // the NaN-safe complement of `up` for the branch below to them)
  if ((x >= ka) & (x < kb)) return;
  if (x >= kb) {
    if (i >= n - 2) return;
    Rec const c = SCALAR ? ld_rec_u(rec, e0 + i + 1) : ld_rec(rec, e0 + i + 1);           // bracket [i+1, i+2]
    double const kc = cvt_keep(ON_EPS ? c.e1 : c.u1);
    if (i + 2 >= n - 1 || kc > x) { ++i; r = c; ka = kb; kb = kc; return; }
    int lo = i + 2, hi, step = 2;
    for (;;) {
      hi = lo + step;
      if (hi >= n - 1) { hi = n - 1; break; }
      if (rec_key<ON_EPS>(rec, e0 + hi) > x) break;
      lo = hi;
      step <<= 1;
    }
    while (hi > lo + 1) {
      int const mid = (lo + hi) >> 1;
      if (rec_key<ON_EPS>(rec, e0 + mid) > x) hi = mid; else lo = mid;
    }
    i = lo;
    r = ld_rec(rec, e0 + i);                              // (each far-move branch ends in its own reload)
    ka = cvt_keep(ON_EPS ? r.e0 : r.u0); kb = cvt_keep(ON_EPS ? r.e1 : r.u1);
  } else {
    if (i <= 0) return;
    Rec const c = SCALAR ? ld_rec_u(rec, e0 + i - 1) : ld_rec(rec, e0 + i - 1);           // bracket [i-1, i]
    double const kc = cvt_keep(ON_EPS ? c.e0 : c.u0);
    if (i - 1 <= 0 || kc <= x) { --i; r = c; kb = ka; ka = kc; return; }
    int hi = i - 1, lo, step = 2;
    for (;;) {
      lo = hi - step;
      if (lo <= 0) { lo = 0; break; }
      if (rec_key<ON_EPS>(rec, e0 + lo) <= x) break;
      hi = lo;
      step <<= 1;
    }
    while (hi > lo + 1) {
      int const mid = (lo + hi) >> 1;
      if (rec_key<ON_EPS>(rec, e0 + mid) > x) hi = mid; else lo = mid;
    }
    i = lo;
    r = ld_rec(rec, e0 + i);
    ka = cvt_keep(ON_EPS ? r.e0 : r.u0); kb = cvt_keep(ON_EPS ? r.e1 : r.u1);
  }
}

// Table descriptors of ONE (gas, channel) pair as the look-up sees them: read from global memory, or
// from a copy the workgroup has staged in LDS (every lane of the workgroup works on the same pair; LDS
// reads are counted by lgkmcnt and stay out of the queue of the curve gathers).
extern __shared__ __attribute__((aligned(16))) unsigned char jur_lds[];

template <bool LDS>
struct PairDesc {
  void const *lvb, *cvb;       // global arrays
  void const *ueb;             // first (u, eps) entry of the pair
  unsigned l0;                 // first level of the pair
  unsigned kbase;              // first curve of the pair (LDS copy starts there)
  __device__ __forceinline__ Lvl lvl(int i) const {
    if constexpr (LDS) return reinterpret_cast<Lvl const *>(jur_lds)[i];
    else return ldg<Lvl>(lvb, l0 + (unsigned)i);
  }
  __device__ __forceinline__ Crv crv(unsigned k) const {
    if constexpr (LDS) return reinterpret_cast<Crv const *>(jur_lds + JUR_TBLNP * sizeof(Lvl))[k - kbase];
    else return ldg<Crv>(cvb, k);
  }
  // 1/(p[i+1] - p[i]) and 1/(T[k+1] - T[k]): formed by the staging loop (LDS), or here with the same division --
  // the same doubles either way (the fused kernel reads its descriptors through L1 and has no staged copy)
  unsigned rp_off, rt_off;     // byte offsets of the two reciprocal arrays in the LDS block
  void const *recb = nullptr;  // bracket records of the pair (set by the kernels that use them)
  __device__ __forceinline__ double rp(int i) const {
    if constexpr (LDS) return reinterpret_cast<double const *>(jur_lds + rp_off)[i];
    else return 1. / (lvl(i + 1).p - lvl(i).p);
  }
  __device__ __forceinline__ double rt(unsigned k) const {
    if constexpr (LDS) return reinterpret_cast<double const *>(jur_lds + rt_off)[k - kbase];
    else return 1. / (crv(k + 1).t - crv(k).t);
  }
};

// EXACT look-up: the reference's bisections probe for probe (locate_id jr_common.h:106-114, locate_tbl_id
// :116-125), for tables whose axes or curves are not sorted.
template <bool LDS>
__device__ __forceinline__ double ega_eps_exact(jur_view_t const &v, jur_int2 const pr, PairDesc<LDS> const &D, double tau, double t,
                                                double u, double p) {
  if (tau < 1e-9) return 0.;
  if (pr.a < 2) return 1.;
  void const *const ueb = D.ueb;
  int ilo = 0, ihi = pr.a - 1;
  while (ihi > ilo + 1) {  // ascending-only bisection, whatever the axis looks like
    int const i = (ihi + ilo) >> 1;
    if (D.lvl(i).p > p) ihi = i; else ilo = i;
  }
  Lvl const l0 = D.lvl(ilo), l1 = D.lvl(ilo + 1);
  if (l0.nt < 2 || l1.nt < 2) return 1.;
  unsigned const k0 = (unsigned)l0.c0, k1 = (unsigned)l1.c0;
  ilo = 0; ihi = l0.nt - 1;
  while (ihi > ilo + 1) {
    int const i = (ihi + ilo) >> 1;
    if (D.crv(k0 + i).t > t) ihi = i; else ilo = i;
  }
  Crv const c00 = D.crv(k0 + ilo), c01_ = D.crv(k0 + ilo + 1);
  if (c00.nu < 2 || c01_.nu < 2) return 1.;
  ilo = 0; ihi = l1.nt - 1;
  while (ihi > ilo + 1) {
    int const i = (ihi + ilo) >> 1;
    if (D.crv(k1 + i).t > t) ihi = i; else ilo = i;
  }
  Crv const c10 = D.crv(k1 + ilo), c11 = D.crv(k1 + ilo + 1);
  if (c10.nu < 2 || c11.nu < 2) return 1.;
  // the four (p,T) corners: u at which the curve reaches eps (get_u, jr_common.h:179-185), then the
  // curve's emissivity at that u plus the segment's column (get_eps, :156-177)
  double const eps = 1 - tau;
  unsigned const e0[4] = {(unsigned)c00.e0, (unsigned)c01_.e0, (unsigned)c10.e0, (unsigned)c11.e0};
  int const n[4] = {c00.nu, c01_.nu, c10.nu, c11.nu};
  double ec[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    Ue a, b;
    ld_pair(ueb, e0[k] + bisect_curve<true>(ueb, e0[k], n[k], eps), a, b);
    double const x = lip((double)a.eps, (double)a.u, (double)b.eps, (double)b.u, eps) + u;
    ld_pair(ueb, e0[k] + bisect_curve<false>(ueb, e0[k], n[k], x), a, b);
    ec[k] = c01(lip((double)a.u, (double)a.eps, (double)b.u, (double)b.eps, x));
  }
  double const eps_p0 = c01(lip(c00.t, ec[0], c01_.t, ec[1], t));
  double const eps_p1 = c01(lip(c10.t, ec[2], c11.t, ec[3], t));
  double const eps_t = c01(lip(l0.p, eps_p0, l1.p, eps_p1, p));
  return (1. - eps_t) / tau;
}

// WARM look-up (sorted tables: every bracket is unique, so any search finds the reference's bracket).
// Search state carried from segment to segment in three packed registers:
//   br = ipr | it0 << 8 | it1 << 16,  ia = idx00 | idx01 << 16,  ib = idx10 | idx11 << 16
// The curve positions kept are those where get_eps ended: the next segment's path emissivity is this
// segment's result, i.e. close to eps(x) on every curve, so its get_u search usually starts inside its
// bracket (-10 % kernel time against resuming from get_u's position).
// The two pressure levels are handled one after the other by a rolled loop, two curves (the temperature
// bracket of the level) at a time: half the curve state is live, 70 VGPRs (62 with RCPB: 8 waves per SIMD), 7 waves per SIMD (-5 %
// against all four curves side by side at 88 VGPRs).
// RCPB (LDS copy present; p and T axes and, as stored in fp32, every curve strictly increasing: no bracket
// has zero width): the three blends divide by multiplying with the reciprocal bracket widths staged in
// LDS (div_rcp), the other nine divisions use div_finite.
// RCPB is the strict-table arithmetic described at lip_slope; with PATH the function returns the NEW path
// transmittance (1 - eps_t, or tau where the reference's look-up answers 1) instead of the segment's
// transmittance (1 - eps_t) / tau -- what the kernels carry and write; the known-answer hook asks for the quotient.
template <bool LDS, bool RCPB, bool PATH = false>
__device__ __forceinline__ double ega_eps_warm(jur_view_t const &v, jur_int2 const pr, PairDesc<LDS> const &D, double tau, double t,
                                               double u, double p, unsigned &br, unsigned &ia, unsigned &ib) {
  static_assert(RCPB || !PATH, "only the strict-table arithmetic carries the path transmittance itself");
  double const one = PATH ? tau : 1.;          // the look-up's "no change" answer
  if (tau < 1e-9) return 0.;
  if (pr.a < 2) return one;
  void const *const ueb = D.ueb;
  int ipr = min((int)(br & 0xffu), pr.a - 2);
  Lvl l0 = D.lvl(ipr), l1 = D.lvl(ipr + 1);
  if ((p < l0.p) | (p >= l1.p)) {
    while (p < l0.p && ipr > 0) { --ipr; l1 = l0; l0 = D.lvl(ipr); }
    while (p >= l1.p && ipr < pr.a - 2) { ++ipr; l0 = l1; l1 = D.lvl(ipr + 1); }
  }
  br = (br & ~0xffu) | (unsigned)ipr;
  if (l0.nt < 2 || l1.nt < 2) return one;
  unsigned const k0 = (unsigned)l0.c0, k1 = (unsigned)l1.c0;
  int it0 = min((int)((br >> 8) & 0xffu), l0.nt - 2), it1 = min((int)((br >> 16) & 0xffu), l1.nt - 2);
  {
    Crv c00 = D.crv(k0 + it0), c01_ = D.crv(k0 + it0 + 1), c10 = D.crv(k1 + it1), c11 = D.crv(k1 + it1 + 1);
    if ((t < c00.t) | (t >= c01_.t) | (t < c10.t) | (t >= c11.t)) {
      while (t < c00.t && it0 > 0) { --it0; c01_ = c00; c00 = D.crv(k0 + it0); }
      while (t >= c01_.t && it0 < l0.nt - 2) { ++it0; c00 = c01_; c01_ = D.crv(k0 + it0 + 1); }
      while (t < c10.t && it1 > 0) { --it1; c11 = c10; c10 = D.crv(k1 + it1); }
      while (t >= c11.t && it1 < l1.nt - 2) { ++it1; c10 = c11; c11 = D.crv(k1 + it1 + 1); }
    }
    br = (unsigned)ipr | ((unsigned)it0 << 8) | ((unsigned)it1 << 16);
    if (c00.nu < 2 || c01_.nu < 2 || c10.nu < 2 || c11.nu < 2) return one;
  }
  // RCPB clamps with the clamp modifier (fma_c01 / add_c01), which would turn a NaN into 0: a NaN among the inputs (the
  // tables hold none) is answered here with what the comparisons of c01 would have handed through
  if (RCPB && (tau != tau || t != t || u != u || p != p)) return __builtin_nan("");
  double const eps = 1 - tau;
  double eps_p0 = 0, eps_p1 = 0;
  // (the records of BOTH levels requested before any is used: 92 VGPRs -- 40.9 ms at 5 wavefronts per SIMD, 101 ms with the
  // excess in scratch at 6, against 35.0: profiles/r04_ega_bracket_records_experiment.json)
#pragma unroll 1
  for (int h = 0; h < 2; h++) {  // pressure level l0, then l1
    unsigned const kc = h ? k1 + (unsigned)it1 : k0 + (unsigned)it0;
    Crv const ca = D.crv(kc), cb = D.crv(kc + 1);
    unsigned const packed = h ? ib : ia;
    unsigned const e0[2] = {(unsigned)ca.e0, (unsigned)cb.e0};
    int const n[2] = {ca.nu, cb.nu};
    int i[2] = {(int)(packed & 0xffffu), (int)(packed >> 16)};
#pragma unroll
    for (int k = 0; k < 2; k++) i[k] = min(i[k], n[k] - 2);
    double x[2], ec[2];
    // get_u (jr_common.h:179-185): u at which the curve reaches eps; get_eps (:156-177): the curve's
    // emissivity at that u plus the segment's column -- the column only grows, so the second search
    // starts where the first ended
    if constexpr (RCPB) {   // one record per bracket: keys and both slopes in one fetch
      Rec r[2];
      ld_rec2(D.recb, e0[0] + i[0], e0[1] + i[1], r[0], r[1]);      // both fetches in flight, then one curve after the other
      // (carrying the four table values of a record as doubles, converted where the record is fetched, costs four more
      // registers than the floats with the two keys the searches hold: 65 VGPRs, the eighth wavefront gone, 36.5 against
      // 35.0 ms -- with the shorter chain of fetches the eighth wavefront matters again)
#pragma unroll
      for (int k = 0; k < 2; k++) {
        double ka, kb;
        seek_rec<true, false>(D.recb, e0[k], n[k], eps, i[k], r[k], ka, kb);
        double const ya = cvt_keep(r[k].u0);
        x[k] = lip_slope(ka, ya, r[k].du_de, eps) + u;
        ka = ya; kb = cvt_keep(r[k].u1);
        seek_rec<false, true>(D.recb, e0[k], n[k], x[k], i[k], r[k], ka, kb);
        ec[k] = lip_slope_c01(ka, (double)r[k].e0, r[k].de_du, x[k]);
      }
    } else {
      Ue a[2], b[2];
#pragma unroll
      for (int k = 0; k < 2; k++) ld_pair(ueb, e0[k] + i[k], a[k], b[k]);
#pragma unroll
      for (int k = 0; k < 2; k++) seek_curve<true>(ueb, e0[k], n[k], eps, i[k], a[k], b[k]);
#pragma unroll
      for (int k = 0; k < 2; k++) x[k] = lip((double)a[k].eps, (double)a[k].u, (double)b[k].eps, (double)b[k].u, eps) + u;
#pragma unroll
      for (int k = 0; k < 2; k++) seek_curve<false>(ueb, e0[k], n[k], x[k], i[k], a[k], b[k]);
#pragma unroll
      for (int k = 0; k < 2; k++) ec[k] = c01(lip((double)a[k].u, (double)a[k].eps, (double)b[k].u, (double)b[k].eps, x[k]));
    }
    unsigned const last = (unsigned)i[0] | ((unsigned)i[1] << 16);
    if (h) ib = last; else ia = last;
    double e;
    if constexpr (RCPB) e = lip_mulr_c01(ca.t, ec[0], ec[1], t, D.rt(kc));
    else e = c01(lip(ca.t, ec[0], cb.t, ec[1], t));
    if (h) eps_p1 = e; else eps_p0 = e;
  }
  if constexpr (RCPB) {
    // the two level pressures are read from LDS again rather than kept through both levels: 4 VGPRs, which is what
    // kept the kernel at 7 waves per SIMD with the keys held as doubles (round 2; 8 waves at 62 VGPRs since the slopes)
    int q = ipr;
    asm volatile("" : "+v"(q));
    double const tau_new = 1. - lip_mulr_c01(D.lvl(q).p, eps_p0, eps_p1, p, D.rp(q));
    if constexpr (PATH) return tau_new;
    else return div_finite(tau_new, tau);
  }
  return (1. - c01(lip(l0.p, eps_p0, l1.p, eps_p1, p))) / tau;
}

// The same look-up by the four lanes of a quad, one (p, T) corner curve each (fused kernel: the chain's latency is
// what counts there, and the four curve searches + interpolations are its longest part).  All four lanes hold the
// chain's inputs and run the bracket searches redundantly; lane q takes curve q = 2 * level + temperature side,
// the four curve emissivities are exchanged with DPP moves and every lane forms the blends -- the operations of
// ega_eps_warm<false, false> in the same order, hence the same doubles.  State: br as there, ix = this lane's
// position in its own curve.
// FAST: the strict-table arithmetic of ega_eps_warm<.., true, true> (lip_slope, lip_mulr with the reciprocal widths
// formed here by division -- the same doubles as the staged ones), returning the new path transmittance: the same
// doubles as the batched kernel.  Otherwise the reference's arithmetic, returning the segment's transmittance.
template <bool FAST>
__device__ __forceinline__ double ega_eps_warm_quad(jur_view_t const &v, jur_int2 const pr, PairDesc<false> const &D, double tau,
                                                    double t, double u, double p, unsigned &br, unsigned &ix) {
  double const one = FAST ? tau : 1.;
  if (tau < 1e-9) return 0.;
  if (pr.a < 2) return one;
  void const *const ueb = D.ueb;
  int ipr = min((int)(br & 0xffu), pr.a - 2);
  Lvl l0 = D.lvl(ipr), l1 = D.lvl(ipr + 1);
  if ((p < l0.p) | (p >= l1.p)) {
    while (p < l0.p && ipr > 0) { --ipr; l1 = l0; l0 = D.lvl(ipr); }
    while (p >= l1.p && ipr < pr.a - 2) { ++ipr; l0 = l1; l1 = D.lvl(ipr + 1); }
  }
  br = (br & ~0xffu) | (unsigned)ipr;
  if (l0.nt < 2 || l1.nt < 2) return one;
  unsigned const k0 = (unsigned)l0.c0, k1 = (unsigned)l1.c0;
  int it0 = min((int)((br >> 8) & 0xffu), l0.nt - 2), it1 = min((int)((br >> 16) & 0xffu), l1.nt - 2);
  Crv c00 = D.crv(k0 + it0), c01_ = D.crv(k0 + it0 + 1), c10 = D.crv(k1 + it1), c11 = D.crv(k1 + it1 + 1);
  if ((t < c00.t) | (t >= c01_.t) | (t < c10.t) | (t >= c11.t)) {
    while (t < c00.t && it0 > 0) { --it0; c01_ = c00; c00 = D.crv(k0 + it0); }
    while (t >= c01_.t && it0 < l0.nt - 2) { ++it0; c00 = c01_; c01_ = D.crv(k0 + it0 + 1); }
    while (t < c10.t && it1 > 0) { --it1; c11 = c10; c10 = D.crv(k1 + it1); }
    while (t >= c11.t && it1 < l1.nt - 2) { ++it1; c10 = c11; c11 = D.crv(k1 + it1 + 1); }
  }
  br = (unsigned)ipr | ((unsigned)it0 << 8) | ((unsigned)it1 << 16);
  if (c00.nu < 2 || c01_.nu < 2 || c10.nu < 2 || c11.nu < 2) return one;
  int const q = threadIdx.x & 3;
  Crv const mine = (q == 0) ? c00 : (q == 1) ? c01_ : (q == 2) ? c10 : c11;
  unsigned const e0 = (unsigned)mine.e0;
  int const n = mine.nu;
  int i = min((int)ix, n - 2);
  double const eps = 1 - tau;
  if constexpr (FAST) {   // bracket records (round 4): one fetch for the curve's keys and both slopes -- the same doubles
    bool const nan_in = (tau != tau || t != t || u != u || p != p);   // as ega_eps_warm: clamp modifiers below
    Rec r = ld_rec(D.recb, e0 + i);
    double ka, kb;
    seek_rec<true, false, false>(D.recb, e0, n, eps, i, r, ka, kb);
    double const ya = (double)r.u0;
    double const x = lip_slope(ka, ya, r.du_de, eps) + u;
    ka = ya; kb = (double)r.u1;
    seek_rec<false, true, false>(D.recb, e0, n, x, i, r, ka, kb);
    double const ec = lip_slope_c01(ka, (double)r.e0, r.de_du, x);
    ix = (unsigned)i;
    double const ec0 = quad_bcast<0>(ec), ec1 = quad_bcast<1>(ec), ec2 = quad_bcast<2>(ec), ec3 = quad_bcast<3>(ec);
    double const eps_p0 = lip_mulr_c01(c00.t, ec0, ec1, t, 1. / (c01_.t - c00.t));
    double const eps_p1 = lip_mulr_c01(c10.t, ec2, ec3, t, 1. / (c11.t - c10.t));
    double const tau_new = 1. - lip_mulr_c01(l0.p, eps_p0, eps_p1, p, 1. / (l1.p - l0.p));
    return nan_in ? __builtin_nan("") : tau_new;
  } else {
    Ue a, b;
    ld_pair(ueb, e0 + i, a, b);
    seek_curve<true>(ueb, e0, n, eps, i, a, b);
    double const x = lip((double)a.eps, (double)a.u, (double)b.eps, (double)b.u, eps) + u;
    seek_curve<false>(ueb, e0, n, x, i, a, b);
    double const ec = c01(lip((double)a.u, (double)a.eps, (double)b.u, (double)b.eps, x));
    ix = (unsigned)i;
    double const ec0 = quad_bcast<0>(ec), ec1 = quad_bcast<1>(ec), ec2 = quad_bcast<2>(ec), ec3 = quad_bcast<3>(ec);
    double const eps_p0 = c01(lip(c00.t, ec0, c01_.t, ec1, t));
    double const eps_p1 = c01(lip(c10.t, ec2, c11.t, ec3, t));
    return (1. - c01(lip(l0.p, eps_p0, l1.p, eps_p1, p))) / tau;
  }
}

// ---- Curtis-Godson look-up (FORMOD 1) ---------------------------------------------------------------------------
// The gas's transmittance of the path up to and including a segment, read off the tables at the Curtis-Godson means
// of that path: t = cgt, u = cgu (the whole column so far), p = cgp.  The brackets and the two blends are those of
// ega_eps (jr_common.h:241-246, :259-265); the four corners are c01(get_eps(curve, cgu)) -- one forward evaluation per
// curve where the emissivity-growth look-up inverts the curve first (get_u) and then evaluates it.  Answers 0 once the
// path has gone opaque (tau < 1e-9, :239) and tau, "no change", where ega_eps answers 1 (no table, nt < 2, nu < 2).
// The result is NOT limited to tau: a Curtis-Godson path transmittance may rise from one segment to the next.
//
// cga_tau_exact: the reference's bisections probe for probe and its divisions operand for operand (any table).
template <bool LDS>
__device__ __forceinline__ double cga_tau_exact(jur_int2 const pr, PairDesc<LDS> const &D, double tau, double t, double u, double p) {
  if (tau < 1e-9) return 0.;
  if (pr.a < 2) return tau;
  void const *const ueb = D.ueb;
  int ilo = 0, ihi = pr.a - 1;
  while (ihi > ilo + 1) {
    int const i = (ihi + ilo) >> 1;
    if (D.lvl(i).p > p) ihi = i; else ilo = i;
  }
  Lvl const l0 = D.lvl(ilo), l1 = D.lvl(ilo + 1);
  if (l0.nt < 2 || l1.nt < 2) return tau;
  unsigned const k0 = (unsigned)l0.c0, k1 = (unsigned)l1.c0;
  ilo = 0; ihi = l0.nt - 1;
  while (ihi > ilo + 1) {
    int const i = (ihi + ilo) >> 1;
    if (D.crv(k0 + i).t > t) ihi = i; else ilo = i;
  }
  Crv const c00 = D.crv(k0 + ilo), c01_ = D.crv(k0 + ilo + 1);
  if (c00.nu < 2 || c01_.nu < 2) return tau;
  ilo = 0; ihi = l1.nt - 1;
  while (ihi > ilo + 1) {
    int const i = (ihi + ilo) >> 1;
    if (D.crv(k1 + i).t > t) ihi = i; else ilo = i;
  }
  Crv const c10 = D.crv(k1 + ilo), c11 = D.crv(k1 + ilo + 1);
  if (c10.nu < 2 || c11.nu < 2) return tau;
  unsigned const e0[4] = {(unsigned)c00.e0, (unsigned)c01_.e0, (unsigned)c10.e0, (unsigned)c11.e0};
  int const n[4] = {c00.nu, c01_.nu, c10.nu, c11.nu};
  double ec[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    Ue a, b;
    ld_pair(ueb, e0[k] + bisect_curve<false>(ueb, e0[k], n[k], u), a, b);
    ec[k] = c01(lip((double)a.u, (double)a.eps, (double)b.u, (double)b.eps, u));
  }
  double const eps_p0 = c01(lip(c00.t, ec[0], c01_.t, ec[1], t));
  double const eps_p1 = c01(lip(c10.t, ec[2], c11.t, ec[3], t));
  return 1. - c01(lip(l0.p, eps_p0, l1.p, eps_p1, p));
}

// cga_tau_warm: sorted tables, search state (br, ia, ib) carried as in ega_eps_warm -- the column only grows along a
// ray, so the curve searches move one way.  Without RCPB the reference's divisions (the same doubles as
// cga_tau_exact); with RCPB the strict-table arithmetic described at lip_slope: bracket records, the curve's slope,
// reciprocal widths for the blends -- the forward half of ega_eps_warm<.., true, true>.
template <bool LDS, bool RCPB>
__device__ __forceinline__ double cga_tau_warm(jur_int2 const pr, PairDesc<LDS> const &D, double tau, double t, double u, double p,
                                               unsigned &br, unsigned &ia, unsigned &ib) {
  if (tau < 1e-9) return 0.;
  if (pr.a < 2) return tau;
  void const *const ueb = D.ueb;
  int ipr = min((int)(br & 0xffu), pr.a - 2);
  Lvl l0 = D.lvl(ipr), l1 = D.lvl(ipr + 1);
  if ((p < l0.p) | (p >= l1.p)) {
    while (p < l0.p && ipr > 0) { --ipr; l1 = l0; l0 = D.lvl(ipr); }
    while (p >= l1.p && ipr < pr.a - 2) { ++ipr; l0 = l1; l1 = D.lvl(ipr + 1); }
  }
  br = (br & ~0xffu) | (unsigned)ipr;
  if (l0.nt < 2 || l1.nt < 2) return tau;
  unsigned const k0 = (unsigned)l0.c0, k1 = (unsigned)l1.c0;
  int it0 = min((int)((br >> 8) & 0xffu), l0.nt - 2), it1 = min((int)((br >> 16) & 0xffu), l1.nt - 2);
  {
    Crv c00 = D.crv(k0 + it0), c01_ = D.crv(k0 + it0 + 1), c10 = D.crv(k1 + it1), c11 = D.crv(k1 + it1 + 1);
    if ((t < c00.t) | (t >= c01_.t) | (t < c10.t) | (t >= c11.t)) {
      while (t < c00.t && it0 > 0) { --it0; c01_ = c00; c00 = D.crv(k0 + it0); }
      while (t >= c01_.t && it0 < l0.nt - 2) { ++it0; c00 = c01_; c01_ = D.crv(k0 + it0 + 1); }
      while (t < c10.t && it1 > 0) { --it1; c11 = c10; c10 = D.crv(k1 + it1); }
      while (t >= c11.t && it1 < l1.nt - 2) { ++it1; c10 = c11; c11 = D.crv(k1 + it1 + 1); }
    }
    br = (unsigned)ipr | ((unsigned)it0 << 8) | ((unsigned)it1 << 16);
    if (c00.nu < 2 || c01_.nu < 2 || c10.nu < 2 || c11.nu < 2) return tau;
  }
  // (as ega_eps_warm: the clamp modifiers below would turn a NaN into 0; tau is not among their operands -- past the
  // gate the rule does not use it, and a NaN there changes nothing in the reference's arithmetic either)
  if (RCPB && (t != t || u != u || p != p)) return __builtin_nan("");
  double eps_p0 = 0, eps_p1 = 0;
#pragma unroll 1
  for (int h = 0; h < 2; h++) {  // pressure level l0, then l1: two curves live at a time, as in ega_eps_warm
    unsigned const kc = h ? k1 + (unsigned)it1 : k0 + (unsigned)it0;
    Crv const ca = D.crv(kc), cb = D.crv(kc + 1);
    unsigned const packed = h ? ib : ia;
    unsigned const e0[2] = {(unsigned)ca.e0, (unsigned)cb.e0};
    int const n[2] = {ca.nu, cb.nu};
    int i[2] = {(int)(packed & 0xffffu), (int)(packed >> 16)};
#pragma unroll
    for (int k = 0; k < 2; k++) i[k] = min(i[k], n[k] - 2);
    double ec[2];
    if constexpr (RCPB) {
      Rec r[2];
      ld_rec2(D.recb, e0[0] + i[0], e0[1] + i[1], r[0], r[1]);
#pragma unroll
      for (int k = 0; k < 2; k++) {
        double ka, kb;
        seek_rec<false, false>(D.recb, e0[k], n[k], u, i[k], r[k], ka, kb);
        ec[k] = lip_slope_c01(ka, (double)r[k].e0, r[k].de_du, u);
      }
    } else {
      Ue a[2], b[2];
#pragma unroll
      for (int k = 0; k < 2; k++) ld_pair(ueb, e0[k] + i[k], a[k], b[k]);
#pragma unroll
      for (int k = 0; k < 2; k++) seek_curve<false>(ueb, e0[k], n[k], u, i[k], a[k], b[k]);
#pragma unroll
      for (int k = 0; k < 2; k++) ec[k] = c01(lip((double)a[k].u, (double)a[k].eps, (double)b[k].u, (double)b[k].eps, u));
    }
    unsigned const last = (unsigned)i[0] | ((unsigned)i[1] << 16);
    if (h) ib = last; else ia = last;
    double e;
    if constexpr (RCPB) e = lip_mulr_c01(ca.t, ec[0], ec[1], t, D.rt(kc));
    else e = c01(lip(ca.t, ec[0], cb.t, ec[1], t));
    if (h) eps_p1 = e; else eps_p0 = e;
  }
  if constexpr (RCPB) {
    int q = ipr;
    asm volatile("" : "+v"(q));           // the level pressures read again, not kept through both levels (ega_eps_warm)
    return 1. - lip_mulr_c01(D.lvl(q).p, eps_p0, eps_p1, p, D.rp(q));
  }
  return 1. - c01(lip(l0.p, eps_p0, l1.p, eps_p1, p));
}

// One segment of a ray under FORMOD 1: the running sums of curtis_godson() (jr_common.h:455-473; products and sums
// rounded separately, the file is compiled without contraction), the means by true divisions, the look-up.  With
// nothing of the gas on the path so far (w == 0: the means would be 0 / 0) the path transmittance stays as it is.
template <bool WARM, bool LDS, bool RCPB>
__device__ __forceinline__ double cga_segment(jur_int2 const pr, PairDesc<LDS> const &D, double tau, double t, double u, double p,
                                              double &sa, double &sb, double &sw, unsigned &br, unsigned &ia, unsigned &ib) {
  double const up = u * p, ut = u * t;
  sa = sa + up; sb = sb + ut; sw = sw + u;
  if (tau < 1e-9) return 0.;
  if (sw == 0.) return tau;
  double const cgp = sa / sw, cgt = sb / sw;
  if constexpr (WARM) return cga_tau_warm<LDS, RCPB>(pr, D, tau, cgt, sw, cgp, br, ia, ib);
  else return cga_tau_exact<LDS>(pr, D, tau, cgt, sw, cgp);
}

// ---------------------------------------------------------------------------------------
// continua; the channel-only factors come precomputed in jur_chan_t
// ---------------------------------------------------------------------------------------
// a / C for a compile-time constant C: the quotient through r = RN(1/C) (div_rcp), folded by the compiler
struct CO2_DEN { static constexpr double v = JUR_AVOGADRO * 1000 * JUR_P0; };
struct P0_DEN { static constexpr double v = JUR_P0; };
struct T36_DEN { static constexpr double v = 296. - 260.; };
struct TR_DEN { static constexpr double v = 296.; };
template <class C>
__device__ __forceinline__ double div_const(double a) { return div_rcp(a, C::v, 1. / C::v); }

__device__ __forceinline__ double ctm_co2(jur_chan_t const &ch, double p, double t, double u) {
  double const dt230 = t - 230;
  double const dt260 = t - 260;
  double const dt296 = t - 296;
  double const ctw = dt260 * 5.050505e-4 * dt296 * ch.co2_cw230 - dt230 * 9.259259e-4 * dt296 * ch.co2_cw260
                   + dt230 * 4.208754e-4 * dt260 * ch.co2_cw296;
  return div_const<CO2_DEN>(u * p * ctw);
}

// ratio^y for a per-channel constant ratio: exp(y ln ratio) with ln ratio = hi + lo prepared on the host
// (64-bit logarithm) and the product y ln ratio carried with its rounding error -- about 1 ulp like the
// library's pow, which spends most of its ~180 instructions on that logarithm.
template <class Tab>
__device__ __forceinline__ double pow_const(Tab const &tab, double lnr_hi, double lnr_lo, double y) {
  double const ph = y * lnr_hi;
  double const pl = __builtin_fma(y, lnr_hi, -ph) + y * lnr_lo;
  double const e = exp_tab(tab, ph);
  return __builtin_fma(e, pl, e);
}

// 1 / t for the continua of one segment: 296/T, 0.7193876/T, 273/T and 1/T (jr_common.h:352-355, 374, 388) share
// it as multiplications.  rcp + two Newton steps: within an ulp of the correctly rounded reciprocal, so every product
// below is within ~2 ulp of the reference's quotient -- 1e-16 relative where the contract is 1e-6 -- for 5
// instructions instead of 3 .. 4 full divisions (~45).  (Round 2 measured the bit-identical form of this sharing
// slower because of two spilled registers; without the correctly-rounded residual steps it is not.)
__device__ __forceinline__ double rcp_t(double t) {
  double r = __builtin_amdgcn_rcp(t);
  r = __builtin_fma(r, __builtin_fma(-t, r, 1.0), r);
  return __builtin_fma(r, __builtin_fma(-t, r, 1.0), r);
}

// tanh(x) for the x = 0.7193876 nu / T > 0 of the H2O continuum (jr_common.h:354): (1 - e) / (1 + e) with
// e = exp(-2x) -- one exp and one division instead of the library's tanh (which branches on the size of x, costs about
// twice as much and keeps a second set of polynomial coefficients in registers across the segment loop).  1 - e loses
// log2(1 / 2x) bits to cancellation: relative error ~1e-16 / 2x, i.e. <= 2e-15 for nu >= 100 cm^-1 at any T <= 1000 K
// and 2e-14 for a channel at 1 cm^-1 -- eight orders inside the contract.
template <class Tab>
__device__ __forceinline__ double tanh_pos(Tab const &tab, double x) {
  double const e = exp_tab(tab, -2. * x);
  return div_finite(1. - e, 1. + e);
}

template <class Tab>
__device__ __forceinline__ double ctm_h2o(Tab const &tab, jur_chan_t const &ch, double p, double t, double rt, double q, double u) {
  double const y = div_const<T36_DEN>(296. - t);
  double const ctwslf = ch.h2o_sc * pow_const(tab, ch.h2o_lnr_hi, ch.h2o_lnr_lo, y);
  double const x = .7193876 * rt * ch.nu;
  double const a1 = ch.nu * u * tanh_pos(tab, x);
  double const a2 = 296. * rt;
  double const a3 = div_const<P0_DEN>(p) * (q * ctwslf + (1 - q) * ch.h2o_ctwfrn) * 1e-20;
  return a1 * a2 * a3;
}

template <class Tab>
__device__ __forceinline__ double ctm_n2(Tab const &tab, jur_chan_t const &ch, double p, double t, double rt) {
  double const q_n2 = 0.79, t0 = 273, tr = 296;
  double const pr = div_const<P0_DEN>(p), s = t0 * rt;
  return 0.1 * pr * pr * s * s * exp_tab(tab, ch.n2_beta * (1 / tr - rt)) * q_n2 * ch.n2_b
         * (q_n2 + (1 - q_n2) * (1.294 - div_const<TR_DEN>(0.4545 * t)));
}

template <class Tab>
__device__ __forceinline__ double ctm_o2(Tab const &tab, jur_chan_t const &ch, double p, double t, double rt) {
  double const q_o2 = 0.21, t0 = 273, tr = 296;
  double const pr = div_const<P0_DEN>(p), s = t0 * rt;
  return 0.1 * pr * pr * s * s * exp_tab(tab, ch.o2_beta * (1 / tr - rt)) * q_o2 * ch.o2_b;
}

__device__ __forceinline__ double planck_src(double const *__restrict__ sr, double t) {
  // 0.25 K grid from 100 K (locate_st, jr_common.h:82-84).  Upstream has no range check and reads
  // outside the table for T outside [100, 400) K; here the index is clamped (end intervals extrapolate).
  int const it = min(max((int)(4 * t) - 400, 0), TBLNS - 2);
  // grid points 100 + it * 300 / 1200 are multiples of 0.25: exact doubles, and the bracket width
  // st1 - st0 is exactly 0.25, so the interpolation's division is the exact multiplication by 4
  double const st0 = 100 + 0.25 * (double)it;
  return sr[it] + (t - st0) * (sr[it + 1] - sr[it]) * 4.0;
}

// Transmittance of all gases over ONE segment (apply_ega_core's product of the per-gas segment transmittances,
// jr_common.h:270-280) from the products of the gases' PATH transmittances after this segment (pcur) and after
// the previous one (pprev): one division per (channel, segment) instead of one per gas.  A gas whose path has
// gone opaque (path transmittance 0: jr_common.h:239 answers 0 from there on) makes pcur, and from the next segment
// pprev, 0: the reference's product is 0 there too.  (A pprev below 1e-280 -- twenty gases each within a hair of
// opaque -- is treated like 0: the ray's own transmittance is below it, nothing it could still add is representable.)
__device__ __forceinline__ double segment_tau_gas(double pcur, double pprev) {
  return (pprev > 1e-280) ? div_finite(pcur, pprev) : 0.;
}

// radiance update of one segment (new_obs_core, jr_common.h:293-300)
template <class Tab>
__device__ __forceinline__ void new_obs_step(Tab const &tab, double tau_gas, double beta_ds, double src, double &rad, double &tau) {
  if (tau_gas > 1e-50) {
    double const eps = 1. - tau_gas * exp_tab(tab, -beta_ds);
    rad += src * eps * tau;
    tau *= (1. - eps);
  }
}

// after the last segment: surface emission if the ray hit the ground (add_surface_core, jr_common.h:227-234),
// brightness temperature if asked for (brightness_core, :187-190)
__device__ __forceinline__ void ray_epilogue(double const *__restrict__ sr, double nu, double tsurf, int write_bbt, double &rad,
                                             double const tau) {
  if (tsurf > 0.) rad += planck_src(sr, tsurf) * tau;
  if (write_bbt) rad = JUR_C2 * nu / log1p((JUR_C1 * nu * nu * nu) / rad);
}

// ---------------------------------------------------------------------------------------
// Workgroup -> (ray block, item) for the kernels whose workgroups of one ray block share its LOS rows: the hardware
// deals workgroups to the 8 XCDs round robin (b % 8), each XCD has its own L2, so the `nitem` workgroups of a ray block
// follow each other on ONE XCD: b -> xcd = b % 8, s = b / 8, ray block = (s / nitem) * 8 + xcd, item = s % nitem --
// eight ray blocks in flight, one per XCD.  The last, incomplete group of k < 8 ray blocks would leave 8 - k XCDs idle for
// as long as a whole group takes (a launch of 49 ray blocks x 7134 pairs: 12 % of its time): there the XCDs x with
// x % k == j share ray block j and split its items between them.  Placement only; every (ray block, item) runs once.
// ---------------------------------------------------------------------------------------
struct BlockItem { int rb, item; };
__host__ __device__ inline unsigned xcd_grid(int nrb, int nitem) {
  int const full = nrb >> 3, k = nrb & 7;
  return (unsigned)(full * 8 * nitem + (k ? 8 * ((nitem + (8 / k) - 1) / (8 / k)) : 0));
}
__device__ __forceinline__ BlockItem xcd_block_item(int b, int nrb, int nitem) {      // rb < 0: nothing to do
  int const full = nrb >> 3, k = nrb & 7, nfull = full * 8 * nitem;
  if (b < nfull) {
    int const xcd = b & 7, s = b >> 3;
    return {(s / nitem) * 8 + xcd, s - (s / nitem) * nitem};
  }
  if (k == 0) return {-1, 0};
  int const bb = b - nfull, xcd = bb & 7, s = bb >> 3;
  int const j = xcd % k, cj = (8 - j + k - 1) / k, q = xcd / k;          // XCDs j, j + k, j + 2k .. share ray block j
  int const item = s * cj + q;
  return {item < nitem ? full * 8 + j : -1, item};
}

// Stage the level and curve descriptors (16 B each) of one (gas, channel) pair in LDS, once per workgroup, with
// the reciprocal widths of the p and T brackets when the tables are strictly increasing (RCPB).  Ends in a barrier.
template <bool LDS, bool RCPB>
__device__ __forceinline__ void stage_pair(jur_view_t const &v, jur_int2 const pd, PairDesc<LDS> &D) {
  if (LDS) {
    Lvl const *const gl = reinterpret_cast<Lvl const *>(v.lvl) + pd.b;
    Lvl const first = gl[0], last = gl[pd.a - 1];
    D.kbase = (unsigned)first.c0;
    int const ncrv = last.c0 + last.nt - first.c0;
    Lvl *const sl = reinterpret_cast<Lvl *>(jur_lds);
    Crv *const sc = reinterpret_cast<Crv *>(jur_lds + JUR_TBLNP * sizeof(Lvl));
    Crv const *const gc = reinterpret_cast<Crv const *>(v.crv) + first.c0;
    for (int i = threadIdx.x; i < pd.a; i += blockDim.x) sl[i] = gl[i];
    for (int i = threadIdx.x; i < ncrv; i += blockDim.x) sc[i] = gc[i];
    if (RCPB) {  // reciprocal widths of the p and T brackets (entries that straddle two axes are never used)
      D.rp_off = (unsigned)((JUR_TBLNP + v.max_pair_curves) * 16);
      D.rt_off = D.rp_off + (unsigned)(JUR_TBLNP * 8);
      double *const rp = reinterpret_cast<double *>(jur_lds + D.rp_off), *const rt = reinterpret_cast<double *>(jur_lds + D.rt_off);
      for (int i = threadIdx.x; i + 1 < pd.a; i += blockDim.x) rp[i] = 1. / (gl[i + 1].p - gl[i].p);
      for (int i = threadIdx.x; i + 1 < ncrv; i += blockDim.x) rt[i] = 1. / (gc[i + 1].t - gc[i].t);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------
// along-path integration in two kernels.  The emissivity-growth recurrence of every (ray, channel,
// gas) triple is an independent sequential chain, so it gets its own lane -- ng x more lanes than
// one lane per (ray, channel), half the registers, 7 - 8 waves per SIMD to hide the dependent table
// loads -- and hands its path transmittance after every segment to the combine kernel through HBM
// (tiles of 64 ray slots, [tile][point][pair][64]).  (A fused single kernel with the gases unrolled in one lane
// was measured 1.7x slower: 166+ VGPRs, 2-3 waves per SIMD.)
//
// jur_ega_kernel: one lane per ray, one (channel, gas) pair per workgroup.  Workgroups that
// share a block of rays are made consecutive on one XCD (they re-read the same p, T, u lines
// from that XCD's L2): b -> xcd = b % 8, s = b / 8, ray block = (s / npair) * 8 + xcd,
// pair = s % npair.  Placement only affects speed.
// ---------------------------------------------------------------------------------------
#ifndef JUR_REC_WAVES
#define JUR_REC_WAVES 7
#endif
template <bool WARM, bool LDS, bool RCPB>
__global__ __launch_bounds__(256, RCPB ? JUR_REC_WAVES : 5) void jur_ega_kernel(jur_view_t v, jur_chunk_t c, int nrb) {
  static_assert(WARM || !RCPB, "reciprocal widths need strictly increasing axes");
  int const npair = v.nd * v.ng;
  BlockItem const bi = xcd_block_item((int)blockIdx.x, nrb, npair);
  if (bi.rb < 0) return;
  // (the launch's block order, as in jur_combine_kernel: which ray block the group of workgroups works on, longest paths
  // first; its pairs still follow each other on one XCD.  With an order the grid covers whole blocks: r < c.n is tested.)
  int const rb = ordered_block<1>(c.blk_order, bi.rb), pr = bi.item;         // ray block, pair: uniform
  int const d = pr / v.ng, g = pr - d * v.ng;
  int const r = rb * blockDim.x + threadIdx.x;
  int const pair_idx = g * v.nd + d;
  jur_int2 const pd = v.pair[pair_idx];
  if (pd.a < 2) return;                          // no table: transmittance 1, the combine kernel knows
  PairDesc<LDS> D{v.lvl, v.crv, v.ue + v.pair_e0[pair_idx], (unsigned)pd.b, 0u, 0u, 0u};
  if constexpr (RCPB) D.recb = v.rec + v.pair_e0[pair_idx];
  stage_pair<LDS, RCPB>(v, pd, D);
  if (r >= c.n) return;
  // the workspaces are addressed as (wave-uniform pointer into this wavefront's tile) + lane offset
  int const nfield = JUR_F_K + v.nw + v.ng;
  int const tile = __builtin_amdgcn_readfirstlane(r >> 6);
  unsigned const lane = (unsigned)(r & 63);
  size_t const R = (size_t)nfield * 64;                              // doubles from one LOS point to the next
  double const *const los_tile = c.los + (size_t)tile * los_tile_doubles(nfield);
  double const *const los_p = los_tile + JUR_F_P * 64, *const los_t = los_tile + JUR_F_T * 64,
               *const los_u = los_tile + (size_t)(JUR_F_K + v.nw + g) * 64;
  size_t const Re = (size_t)npair * 64;                              // ... and from one point's transmittances to the next
  double *const out = c.eps + eps_tile_point0(c, tile) * Re + (size_t)pr * 64;
  int const np = c.np[r];
  double tau_path = 1.0;
  unsigned br = 0, ia = 0, ib = 0;
  // p and T of a segment -- what the look-up needs first, for its bracket tests -- are requested one segment ahead
  // (4 VGPRs; -1.5 % kernel time); u, needed only after the first curve search, is not: in round 2 it cost a wavefront
  // of occupancy (62.6 vs 60.9 ms), with the slopes it fits (64 VGPRs) and changes nothing (39.5 vs 39.8 ms).  The warm
  // variants without reciprocal widths sit at 70 VGPRs and keep loading at the point of use.
  constexpr bool AHEAD = RCPB || !WARM;
  double p_next = 0., t_next = 0.;
  if (AHEAD && np > 0) { p_next = ldg<double>(los_p, lane); t_next = ldg<double>(los_t, lane); }

  for (int ip = 0; ip < np; ++ip) {
    size_t const o = (size_t)ip * R;
    double p, t;
    if constexpr (AHEAD) {
      p = p_next; t = t_next;
      if (ip + 1 < np) { p_next = ldg<double>(los_p + o + R, lane); t_next = ldg<double>(los_t + o + R, lane); }
    } else { p = ldg<double>(los_p + o, lane); t = ldg<double>(los_t + o, lane); }
    double const u = ldg<double>(los_u + o, lane);
    // what is carried and written is the gas's transmittance of the path up to and including this segment
    if constexpr (RCPB) tau_path = ega_eps_warm<LDS, true, true>(v, pd, D, tau_path, t, u, p, br, ia, ib);
    else if constexpr (WARM) tau_path *= ega_eps_warm<LDS, false>(v, pd, D, tau_path, t, u, p, br, ia, ib);
    else tau_path *= ega_eps_exact<LDS>(v, pd, D, tau_path, t, u, p);
    st_stream(out + (size_t)ip * Re, lane, tau_path);
  }
}

// jur_cga_kernel: the same launch under FORMOD 1 -- grid, XCD mapping, block order, staged descriptors, tile
// addressing and output plane of jur_ega_kernel; per lane the three running sums of the Curtis-Godson means and one
// look-up at the means per segment (cga_segment) in place of the emissivity-growth recurrence.  The radiance update
// reads the plane unchanged.
template <bool WARM, bool LDS, bool RCPB>
__global__ __launch_bounds__(256, RCPB ? JUR_REC_WAVES : 5) void jur_cga_kernel(jur_view_t v, jur_chunk_t c, int nrb) {
  static_assert(WARM || !RCPB, "reciprocal widths need strictly increasing axes");
  int const npair = v.nd * v.ng;
  BlockItem const bi = xcd_block_item((int)blockIdx.x, nrb, npair);
  if (bi.rb < 0) return;
  int const rb = ordered_block<1>(c.blk_order, bi.rb), pr = bi.item;         // ray block, pair: uniform
  int const d = pr / v.ng, g = pr - d * v.ng;
  int const r = rb * blockDim.x + threadIdx.x;
  int const pair_idx = g * v.nd + d;
  jur_int2 const pd = v.pair[pair_idx];
  if (pd.a < 2) return;                          // no table: transmittance 1, the combine kernel knows
  PairDesc<LDS> D{v.lvl, v.crv, v.ue + v.pair_e0[pair_idx], (unsigned)pd.b, 0u, 0u, 0u};
  if constexpr (RCPB) D.recb = v.rec + v.pair_e0[pair_idx];
  stage_pair<LDS, RCPB>(v, pd, D);
  if (r >= c.n) return;
  int const nfield = JUR_F_K + v.nw + v.ng;
  int const tile = __builtin_amdgcn_readfirstlane(r >> 6);
  unsigned const lane = (unsigned)(r & 63);
  size_t const R = (size_t)nfield * 64;
  double const *const los_tile = c.los + (size_t)tile * los_tile_doubles(nfield);
  double const *const los_p = los_tile + JUR_F_P * 64, *const los_t = los_tile + JUR_F_T * 64,
               *const los_u = los_tile + (size_t)(JUR_F_K + v.nw + g) * 64;
  size_t const Re = (size_t)npair * 64;
  double *const out = c.eps + eps_tile_point0(c, tile) * Re + (size_t)pr * 64;
  int const np = c.np[r];
  double tau_path = 1.0, sa = 0., sb = 0., sw = 0.;
  unsigned br = 0, ia = 0, ib = 0;
  // all three fields feed the sums before anything else: requested together, one segment ahead
  double p_next = 0., t_next = 0., u_next = 0.;
  if (np > 0) { p_next = ldg<double>(los_p, lane); t_next = ldg<double>(los_t, lane); u_next = ldg<double>(los_u, lane); }

  for (int ip = 0; ip < np; ++ip) {
    size_t const o = (size_t)ip * R;
    double const p = p_next, t = t_next, u = u_next;
    if (ip + 1 < np) {
      p_next = ldg<double>(los_p + o + R, lane); t_next = ldg<double>(los_t + o + R, lane); u_next = ldg<double>(los_u + o + R, lane);
    }
    tau_path = cga_segment<WARM, LDS, RCPB>(pd, D, tau_path, t, u, p, sa, sb, sw, br, ia, ib);
    st_stream(out + (size_t)ip * Re, lane, tau_path);
  }
}

// Everything the radiance update reads for one segment, requested together: the LOS fields of the point (one
// contiguous run of the tile) and the path transmittances of the channel's gases, multiplied in the reference's gas
// order (jr_common.h:272-278).  All loads are issued before the first value is used -- one memory latency per segment.
// (Rounds 1-2 loaded each gas's transmittance inside the product loop, and the continua's columns inside their
// branches: the compiler waited for each in turn, seven dependent round trips to HBM per segment, and the kernel sat
// at half the bandwidth it asks for with idle vector units.)  Gases beyond the first eight take a second batch.
struct SegmentIn { double p, t, ds, k, u_co2, q_h2o, u_h2o, pcur; };
__device__ __forceinline__ SegmentIn load_segment(double const *__restrict__ row, double const *__restrict__ trow, unsigned lane,
                                                  int f_k, int f_co2, int f_h2o, int ng, unsigned has_table, bool k_zero) {
  SegmentIn in;
  in.p = ldg<double>(row + JUR_F_P * 64, lane);
  in.t = ldg<double>(row + JUR_F_T * 64, lane);
  in.ds = ldg<double>(row + JUR_F_DS * 64, lane);
  // (k_zero: the tracer wrote no extinction fields, jur_view_t::atm_k_zero; the +0.0 it would have written goes through
  // the same `k * ds` as a loaded one, so beta_ds starts from the same double whatever ds is.  Uniform.)
  in.k = k_zero ? 0.0 : ldg<double>(row + (size_t)f_k * 64, lane);
  in.u_co2 = ldg<double>(row + (size_t)f_co2 * 64, lane);
  in.q_h2o = ldg<double>(row + JUR_F_QH2O * 64, lane);
  in.u_h2o = ldg<double>(row + (size_t)f_h2o * 64, lane);
  double tg[8];
#pragma unroll
  for (int k = 0; k < 8; k++) tg[k] = (k < ng && ((has_table >> k) & 1u)) ? ld_stream(trow + (size_t)k * 64, lane) : 1.0;
  double pcur = 1.0;
#pragma unroll
  for (int k = 0; k < 8; k++) pcur *= tg[k];           // (x * 1.0 == x: absent gases do not change the product)
  for (int g0 = 8; g0 < ng; g0 += 8) {
#pragma unroll
    for (int k = 0; k < 8; k++) tg[k] = (g0 + k < ng && g0 + k < 32 && ((has_table >> (g0 + k)) & 1u)) ? ld_stream(trow + (size_t)(g0 + k) * 64, lane) : 1.0;
#pragma unroll
    for (int k = 0; k < 8; k++) pcur *= tg[k];
  }
  in.pcur = pcur;
  return in;
}

// jur_combine_kernel: one lane per ray, one channel per workgroup: continua, product of the gas
// transmittances in the reference's order, Planck source, radiance update, epilogue.
// (59 VGPRs since the exponentials go through exp_tab: 8 waves per SIMD)
__global__ __launch_bounds__(256, 6) void jur_combine_kernel(jur_view_t v, jur_chunk_t c, int nrb) {
  int const nd = v.nd, ng = v.ng;
  // same XCD-aware order as jur_ega_kernel: the nd workgroups of one ray block follow each other
  // on one XCD and share the block's LOS rows in that L2
  BlockItem const bi = xcd_block_item((int)blockIdx.x, nrb, nd);
  if (bi.rb < 0) return;
  int const rb = ordered_block<1>(c.blk_order, bi.rb), d = bi.item;   // ray block, channel: uniform
  int const r = rb * blockDim.x + threadIdx.x;
  // the channel's source-function table (1201 doubles) is staged in LDS: its two reads per segment are
  // gathers by temperature, everything else this kernel loads is a coalesced stream
  double *const sr = reinterpret_cast<double *>(jur_lds);
  Exp2Lds const e2t{sr + TBLNS};                       // 2^(j/64), 64 doubles behind the source-function table
  {
    double const *const gsr = v.sr + (size_t)d * TBLNS;
    for (int i = threadIdx.x; i < TBLNS; i += blockDim.x) sr[i] = gsr[i];
    if (threadIdx.x < 64) sr[TBLNS + threadIdx.x] = JUR_EXP2_64[threadIdx.x];
    __syncthreads();
  }
  if (r >= c.n) return;
  long const ray = c.order ? (long)c.order[r] : c.first + r;
  int const nfield = JUR_F_K + v.nw + ng;
  int const tile = __builtin_amdgcn_readfirstlane(r >> 6);
  unsigned const lane = (unsigned)(r & 63);
  size_t const R = (size_t)nfield * 64, Re = (size_t)nd * ng * 64;   // doubles from one LOS point to the next
  double const *const los = c.los + (size_t)tile * los_tile_doubles(nfield);
  double const *const epsb = c.eps + eps_tile_point0(c, tile) * Re + (size_t)d * ng * 64;
  jur_chan_t const ch = v.chan[d];
  int const f_k = JUR_F_K + ch.window, f_u = JUR_F_K + v.nw;
  bool const do_co2 = (v.fourbit & 8) && ch.co2_on, do_h2o = (v.fourbit & 4) && ch.h2o_on,
             do_n2 = (v.fourbit & 2) && ch.n2_on, do_o2 = (v.fourbit & 1) && ch.o2_on;
  size_t const oidx = (size_t)ray * nd + d;
  bool const masked = !isfinite(c.rad[oidx]);
  double rad = 0.0, tau = 1.0, pprev = 1.0;
  int const np = c.np[r];
  unsigned has_table = 0;                              // gases with a table for this channel (uniform)
  for (int g = 0; g < ng && g < 32; g++) has_table |= (v.pair[g * nd + d].a >= 2 ? 1u : 0u) << g;
  int const f_co2 = do_co2 ? f_u + v.ig_co2 : JUR_F_P, f_h2o = do_h2o ? f_u + v.ig_h2o : JUR_F_P;   // (a field that always exists when the continuum is off)
  for (int ip = 0; ip < np; ++ip) {
    SegmentIn const in = load_segment(los + (size_t)ip * R, epsb + (size_t)ip * Re, lane, f_k, f_co2, f_h2o, ng, has_table, v.atm_k_zero != 0);
    double beta_ds = in.k * in.ds;
    if (do_co2) beta_ds += ctm_co2(ch, in.p, in.t, in.u_co2);
    double const rt = rcp_t(in.t);
    if (do_h2o) beta_ds += ctm_h2o(e2t, ch, in.p, in.t, rt, in.q_h2o, in.u_h2o);
    if (do_n2) beta_ds += ctm_n2(e2t, ch, in.p, in.t, rt) * in.ds;
    if (do_o2) beta_ds += ctm_o2(e2t, ch, in.p, in.t, rt) * in.ds;
    double const tau_gas = segment_tau_gas(in.pcur, pprev);
    pprev = in.pcur;
    new_obs_step(e2t, tau_gas, beta_ds, planck_src(sr, in.t), rad, tau);
  }
  ray_epilogue(sr, ch.nu, c.tsurf[r], v.write_bbt, rad, tau);
  if (masked) rad = __builtin_nan("");
  c.rad[oidx] = rad;
  c.tau[oidx] = tau;
}

// jur_combine_group_kernel: the same lane program with the channels of a ray block as wavefronts of ONE workgroup --
// wave w works on channel cg * CG + w % CG for the 64 rays of sub-block w / CG (CG = min(nd, 4) channels per group,
// 8 / CG sub-blocks, 6 or 8 waves) -- and a barrier every SYNC segments that keeps the waves within reach of each
// other: the LOS rows of a segment, which every channel reads, are then found in L2 by all but the first reader
// (FETCH_SIZE of the kernel -29 %).  The kernel waits on its dependent chains more than on HBM, so this is worth
// 4 % of its time, not 29 (17.3 against 18.1 ms per 1e6 limb rays); one channel per workgroup remains for nd = 1.
// The wave index is made uniform (readfirstlane) so that the channel constants stay in scalar registers.
// 8 waves per SIMD (56 VGPRs, no scratch): a workgroup is 8 wavefronts, so anything above 64 VGPRs runs three
// workgroups per CU instead of four; 13.1 ms per 1e6 limb rays against 14.7 ms at 69 VGPRs (A/B: -DJUR_COMBINE_WAVES=6)
#ifndef JUR_COMBINE_WAVES
#define JUR_COMBINE_WAVES 8
#endif
__global__ __launch_bounds__(512, JUR_COMBINE_WAVES) void jur_combine_group_kernel(jur_view_t v, jur_chunk_t c, int nsb, int CG, int SYNC) {   // SYNC: mask, see the loop
  int const nd = v.nd, ng = v.ng;
  int const ncg = (nd + CG - 1) / CG, SUB = (int)(blockDim.x >> 6) / CG;
  BlockItem const bi = xcd_block_item((int)blockIdx.x, nsb, ncg);
  if (bi.rb < 0) return;
  // ray super-block, channel group: uniform.  4 / SUB super-blocks of SUB x 64 slots to the block of the launch's block
  // order (jurk_launch_combine passes one only where SUB is 1, 2 or 4)
  int const msb = 4 / SUB, cg = bi.item;
  int const sb = c.blk_order ? __builtin_amdgcn_readfirstlane(c.blk_order[bi.rb / msb]) * msb + bi.rb % msb : bi.rb;
  int const w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);   // uniform: channel constants stay in SGPRs
  int const cw = w % CG, sub = w / CG;
  int const d = cg * CG + cw;
  bool const live_wave = d < nd;
  double *const sr = reinterpret_cast<double *>(jur_lds) + (size_t)cw * TBLNS;
  int *const npmax_sh = reinterpret_cast<int *>(reinterpret_cast<double *>(jur_lds) + (size_t)CG * TBLNS);
  Exp2Lds const e2t{reinterpret_cast<double *>(jur_lds) + (size_t)CG * TBLNS + 2};   // 2^(j/64), 64 doubles
  if (threadIdx.x == 0) *npmax_sh = 0;
  if (threadIdx.x < 64) reinterpret_cast<double *>(jur_lds)[(size_t)CG * TBLNS + 2 + threadIdx.x] = JUR_EXP2_64[threadIdx.x];
  for (int k = 0; k < CG; k++) {
    if (cg * CG + k >= nd) break;
    double const *const gsr = v.sr + (size_t)(cg * CG + k) * TBLNS;
    double *const dst = reinterpret_cast<double *>(jur_lds) + (size_t)k * TBLNS;
    for (int i = threadIdx.x; i < TBLNS; i += blockDim.x) dst[i] = gsr[i];
  }
  __syncthreads();
  int const r = (sb * SUB + sub) * 64 + lane;
  bool const live = live_wave && r < c.n;
  int const np = live ? c.np[r] : 0;
  atomicMax(npmax_sh, np);
  __syncthreads();
  int const npmax = *npmax_sh;
  long const ray = live ? (c.order ? (long)c.order[r] : c.first + r) : 0;
  int const nfield = JUR_F_K + v.nw + ng;
  int const tile = sb * SUB + sub;                                   // (uniform: w is)
  size_t const R = (size_t)nfield * 64, Re = (size_t)nd * ng * 64;   // doubles from one LOS point to the next
  double const *const los = c.los + (size_t)tile * los_tile_doubles(nfield);
  int const dd = live_wave ? d : 0;
  double const *const epsb = c.eps + eps_tile_point0(c, tile) * Re + (size_t)dd * ng * 64;
  jur_chan_t const ch = v.chan[dd];
  int const f_k = JUR_F_K + ch.window, f_u = JUR_F_K + v.nw;
  bool const do_co2 = (v.fourbit & 8) && ch.co2_on, do_h2o = (v.fourbit & 4) && ch.h2o_on,
             do_n2 = (v.fourbit & 2) && ch.n2_on, do_o2 = (v.fourbit & 1) && ch.o2_on;
  size_t const oidx = (size_t)ray * nd + dd;
  bool const masked = live && !isfinite(c.rad[oidx]);
  double rad = 0.0, tau = 1.0, pprev = 1.0;
  unsigned has_table = 0;
  for (int g = 0; g < ng && g < 32; g++) has_table |= (v.pair[g * nd + dd].a >= 2 ? 1u : 0u) << g;
  int const f_co2 = do_co2 ? f_u + v.ig_co2 : JUR_F_P, f_h2o = do_h2o ? f_u + v.ig_h2o : JUR_F_P;   // (a field that always exists when the continuum is off)
  for (int ip = 0; ip < npmax; ++ip) {
    if (ip < np) {
      SegmentIn const in = load_segment(los + (size_t)ip * R, epsb + (size_t)ip * Re, (unsigned)lane, f_k, f_co2, f_h2o, ng, has_table, v.atm_k_zero != 0);
      double beta_ds = in.k * in.ds;
      if (do_co2) beta_ds += ctm_co2(ch, in.p, in.t, in.u_co2);
      double const rt = rcp_t(in.t);
      if (do_h2o) beta_ds += ctm_h2o(e2t, ch, in.p, in.t, rt, in.q_h2o, in.u_h2o);
      if (do_n2) beta_ds += ctm_n2(e2t, ch, in.p, in.t, rt) * in.ds;
      if (do_o2) beta_ds += ctm_o2(e2t, ch, in.p, in.t, rt) * in.ds;
      double const tau_gas = segment_tau_gas(in.pcur, pprev);
      pprev = in.pcur;
      new_obs_step(e2t, tau_gas, beta_ds, planck_src(sr, in.t), rad, tau);
    }
    if ((ip & SYNC) == SYNC) __syncthreads();      // SYNC = 2^k - 1 (0: a barrier after every segment; -1 never matches: none)
  }
  if (!live) return;
  ray_epilogue(sr, ch.nu, c.tsurf[r], v.write_bbt, rad, tau);
  if (masked) rad = __builtin_nan("");
  c.rad[oidx] = rad;
  c.tau[oidx] = tau;
}

// jur_contrib_kernel: the contribution of every emitter (formod TASK contrib) from the transmittance plane the look-up
// kernel has just written -- one lane per (ray, channel, variant), the lane program of jur_combine_kernel with:
//   variant g < ng   only gas g's path transmittance, no extinction, the CO2 / H2O continuum only if g is that emitter,
//                    N2 / O2 as switched: the forward model on the atmosphere with every other q and every k set to 0;
//   variant ng       no gas (tau_gas = 1), the extinction and the N2 / O2 continua: every q set to 0.
// A gas's path transmittance depends on its own column only (ega_eps, jr_common.h:237-268) and the line of sight on p and
// T only, so one trace and one look-up serve all ng + 2 spectra.  Outputs rad_c / tau_c [ng + 1][nr][nd] by ray id.
// Grid: xcd_block_item over (ray block) x (channel, variant), the ng + 1 variants of a channel adjacent: they share the
// source-function table and read the ray block's LOS rows from one L2; each plane entry is read once, non-temporally.
// (8 waves per SIMD: within 64 VGPRs, no scratch -- tests/test_contrib_cpu.py)
__global__ __launch_bounds__(256, 8) void jur_contrib_kernel(jur_view_t v, jur_chunk_t c, int nrb, long nr, double *__restrict__ rad_c,
                                                             double *__restrict__ tau_c) {
  int const nd = v.nd, ng = v.ng, nvar = ng + 1;
  BlockItem const bi = xcd_block_item((int)blockIdx.x, nrb, nd * nvar);
  int const rb = bi.rb;
  if (rb < 0) return;
  int const d = bi.item / nvar, g = bi.item - d * nvar;          // channel, variant (g == ng: extinction): uniform
  int const r = rb * blockDim.x + threadIdx.x;
  double *const sr = reinterpret_cast<double *>(jur_lds);
  Exp2Lds const e2t{sr + TBLNS};
  {
    double const *const gsr = v.sr + (size_t)d * TBLNS;
    for (int i = threadIdx.x; i < TBLNS; i += blockDim.x) sr[i] = gsr[i];
    if (threadIdx.x < 64) sr[TBLNS + threadIdx.x] = JUR_EXP2_64[threadIdx.x];
    __syncthreads();
  }
  if (r >= c.n) return;
  long const ray = c.order ? (long)c.order[r] : c.first + r;
  int const nfield = JUR_F_K + v.nw + ng;
  int const tile = __builtin_amdgcn_readfirstlane(r >> 6);
  unsigned const lane = (unsigned)(r & 63);
  size_t const R = (size_t)nfield * 64, Re = (size_t)nd * ng * 64;
  double const *const los = c.los + (size_t)tile * los_tile_doubles(nfield);
  jur_chan_t const ch = v.chan[d];
  bool const ext = g == ng;
  bool const has = !ext && v.pair[g * nd + d].a >= 2;           // the plane holds this gas's transmittance (else it is 1)
  double const *const epsb = c.eps + eps_tile_point0(c, tile) * Re + ((size_t)d * ng + (ext ? 0 : g)) * 64;
  int const f_k = JUR_F_K + ch.window, f_g = JUR_F_K + v.nw + (ext ? 0 : g);
  bool const do_co2 = !ext && g == v.ig_co2 && (v.fourbit & 8) && ch.co2_on,
             do_h2o = !ext && g == v.ig_h2o && (v.fourbit & 4) && ch.h2o_on,
             do_n2 = (v.fourbit & 2) && ch.n2_on, do_o2 = (v.fourbit & 1) && ch.o2_on;
  bool const masked = !isfinite(c.rad[(size_t)ray * nd + d]);   // the input radiances: combine has not run yet
  double rad = 0.0, tau = 1.0, pprev = 1.0;
  int const np = c.np[r];
  for (int ip = 0; ip < np; ++ip) {
    double const *const row = los + (size_t)ip * R;
    double const p = ldg<double>(row + JUR_F_P * 64, lane), t = ldg<double>(row + JUR_F_T * 64, lane),
                 ds = ldg<double>(row + JUR_F_DS * 64, lane);
    double const k = (ext && !v.atm_k_zero) ? ldg<double>(row + (size_t)f_k * 64, lane) : 0.;   // (no fields written: +0.0)
    double const ug = (do_co2 || do_h2o) ? ldg<double>(row + (size_t)f_g * 64, lane) : 0.;
    double const qh = do_h2o ? ldg<double>(row + JUR_F_QH2O * 64, lane) : 0.;
    double const pcur = has ? ld_stream(epsb + (size_t)ip * Re, lane) : 1.0;
    double beta_ds = k * ds;                                     // (0 for a gas: the extinction is set to 0 there)
    if (do_co2) beta_ds += ctm_co2(ch, p, t, ug);
    double const rt = rcp_t(t);
    if (do_h2o) beta_ds += ctm_h2o(e2t, ch, p, t, rt, qh, ug);
    if (do_n2) beta_ds += ctm_n2(e2t, ch, p, t, rt) * ds;
    if (do_o2) beta_ds += ctm_o2(e2t, ch, p, t, rt) * ds;
    double const tau_gas = ext ? 1.0 : segment_tau_gas(pcur, pprev);
    pprev = pcur;
    new_obs_step(e2t, tau_gas, beta_ds, planck_src(sr, t), rad, tau);
  }
  ray_epilogue(sr, ch.nu, c.tsurf[r], v.write_bbt, rad, tau);
  if (masked) rad = __builtin_nan("");
  size_t const o = ((size_t)g * (size_t)nr + (size_t)ray) * nd + d;
  rad_c[o] = rad;
  tau_c[o] = tau;
}

// ---------------------------------------------------------------------------------------
// jur_pencil_kernel: the whole path of a ray pencil inside ONE workgroup -- for calls of the size the
// reference's callers make (packages of <= NR = 1088 rays, formod.c:100, kernel() jurassic.c:844), which cannot
// fill 256 CUs with one lane per ray and would run the three batched kernels as three serial <= 400-step chains.
//
// A workgroup owns RB rays.  Its wavefronts take roles and hand the line of sight from one to the next through
// LDS, point by point, as it is being traced:
//   wave 0              traces the rays (trace_ray) into a ring of LOS points in LDS -- up to 16 rays per workgroup
//                       with a quad of lanes per ray, one refraction probe each;
//   waves 1 .. NE       the emissivity-growth recurrence of every (ray, channel, gas) chain on the points the tracer
//                       has released -- sorted tables: a quad of lanes per chain, one (p, T) corner curve each
//                       (ega_eps_warm_quad); search state and accumulated transmittance of the chain in LDS;
//                       segment transmittances go to a second ring;
//   waves NE+1 .. +NC   one lane per (ray, channel): continua, product over the gases, Planck source, radiance
//                       update, epilogue -- the body of jur_combine_kernel.
// The roles overlap along the ray: a call takes about as long as its longest ray takes to TRACE, the LOS state
// and the segment transmittances never touch HBM, and nothing is sorted.  Same device functions, same operand
// order, same doubles as the batched kernels (tests compare the two paths bit for bit).
//
// Hand-over: cnt_trace = number of points of every still-running ray that will not change any more (the lanes of
// wave 0 step in lockstep), npr[ray] = 1 + its point count once the ray has left the atmosphere; every consumer wave
// publishes the number of points it has finished.  All counters live in LDS, release/acquire at workgroup scope.
// Every wait is for a wave of the same workgroup that is resident and never waits for the waiter in turn
// (tracer <- combine: ring slot free; ega <- tracer: point released, <- combine: eps slot free; combine <- ega),
// so every wave reaches its exit.
// ---------------------------------------------------------------------------------------
#define PEN_RING 16       // LOS points in flight (power of two)
#define PEN_RINGE 8       // segment transmittances in flight (power of two, <= PEN_RING)
#define PEN_MAXE 8        // at most this many ega / combine waves per workgroup
#define PEN_MAXC 4

// doubles of dynamic LDS in front of the optional profile slab (rings, chain and radiance state, per-ray results,
// the 32-bit state rounded up to whole doubles)
__host__ __device__ inline long pen_lds_doubles(int nd, int ng, int nw, int RB) {
  long const npair = (long)nd * ng, nfield = JUR_F_K + nw + ng, nchain = RB * npair, nitem = (long)RB * nd;
  long const n1 = nchain > 0 ? nchain : 1;
  return (long)PEN_RING * nfield * RB + (long)PEN_RINGE * (npair > 0 ? npair : 1) * RB + n1 + 3 * nitem + RB + (5 * n1 + RB + 1) / 2 + 2;
}

struct PenCtl {            // LDS, one per workgroup
  int cnt_trace, done;
  int cnt_ega[PEN_MAXE];
  int cnt_comb[PEN_MAXC];
};

__device__ __forceinline__ int ld_acq(int *p) { return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st_rel(int *p, int x) { __hip_atomic_store(p, x, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int min_cnt(int *p, int n) {
  int m = ld_acq(p);
  for (int i = 1; i < n; i++) m = min(m, ld_acq(p + i));
  return m;
}
__device__ __forceinline__ bool first_active_lane() {
  return (int)(threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1;
}

// LOS fields of the workgroup's rays in the LDS ring [point % PEN_RING][field][ray]
struct LosRing {
  double *ring;
  PenCtl *ctl;
  int *npr;
  double *tsurf;
  int nfield, RB, r, nc;
  int shift;               // lanes per ray in the tracer wavefront = 1 << shift (ray slot = lane >> shift)
  __device__ __forceinline__ double &at(int field, int ip) const { return ring[((ip & (PEN_RING - 1)) * nfield + field) * RB + r]; }
  __device__ __forceinline__ void put(int field, int ip, double x) const { at(field, ip) = x; }
  __device__ __forceinline__ size_t field_stride() const { return (size_t)RB; }
  __device__ __forceinline__ void begin_point(int ip) const {   // the slot still holds point ip - PEN_RING
    if (ip >= PEN_RING)
      while (min_cnt(ctl->cnt_comb, nc) + PEN_RING <= ip) __builtin_amdgcn_s_sleep(2);
  }
  // Lanes whose rays left the atmosphere in this step have dropped out of the loop; their own announcement
  // (ray_final) may be scheduled after the loop of the others, so a lane that is still stepping says it for them,
  // in its own program order before the release of the next point: they stopped at point np, i.e. have np + 1 points.
  __device__ __forceinline__ void points_final(int np) {
    unsigned long long const cur = __ballot(1);
    unsigned long long gone = running & ~cur;
    running = cur;
    if (first_active_lane()) {
      for (; gone; gone &= gone - 1) {
        int const l = __ffsll((long long)gone) - 1;
        if ((l & ((1 << shift) - 1)) == 0) st_rel(&npr[l >> shift], np + 2);
      }
      st_rel(&ctl->cnt_trace, np);
    }
  }
  __device__ __forceinline__ void ray_final(int n, double ts) const {
    tsurf[r] = ts;
    st_rel(&npr[r], n + 1);
  }
  __device__ __forceinline__ void never_enter(unsigned long long mask) {   // lane number >> shift == ray slot in wave 0
    running = __ballot(1) & ~mask;
    if (first_active_lane())
      for (; mask; mask &= mask - 1) {
        int const l = __ffsll((long long)mask) - 1;
        if ((l & ((1 << shift) - 1)) == 0) st_rel(&npr[l >> shift], 1);
      }
  }
  unsigned long long running;
};

// wait until point ip is released (returns the released count c > ip) or the tracer is through (returns its final
// count, possibly <= ip: no such point)
__device__ __forceinline__ int wait_point(PenCtl *ctl, int ip) {
  for (;;) {
    int c = ld_acq(&ctl->cnt_trace);
    if (c > ip) return c;
    if (ld_acq(&ctl->done)) return ld_acq(&ctl->cnt_trace);
    __builtin_amdgcn_s_sleep(2);
  }
}

// first point of the profile slice with this time stamp (the first search of locate_atm, jr_common.h:130-140)
__device__ __forceinline__ int slice_start(double const *__restrict__ atm_time, int atm_np, double time) {
  int lo = 0, hi = atm_np - 1;
  while (hi > lo + 1) {
    int const i = (lo + hi) / 2;
    if (atm_time[i] < time) lo = i; else hi = i;
  }
  return (0 == lo) ? lo : hi;
}

// atm_cap > 0: the dynamic LDS block ends in room for (7 + ng + nw) rows of atm_cap doubles -- the profile slice of
// the workgroup's rays (time, z, lon, lat, p, T, q[], k[], ln-p slope), copied there when all its rays use the same
// slice.  The tracer's per-step profile gathers (a chain of dependent loads at L2 latency when one wave per SIMD
// has nothing to hide them behind) then stay inside the CU.  Same numbers from another place: same results.
template <bool WARM, bool QUAD>
__global__ __launch_bounds__(1024) void jur_pencil_kernel(jur_view_t v, jur_chunk_t c, int RB, int NE, int NC, int atm_cap) {
  __shared__ double tr_sh[15][64];
  __shared__ PenCtl ctl;
  __shared__ int sl_lo, sl_hi;
  int const nd = v.nd, ng = v.ng, npair = nd * ng, nfield = JUR_F_K + v.nw + ng;
  int const nchain = RB * npair, nitem = RB * nd;
  // dynamic LDS: rings, chain state, per-(ray, channel) radiance state, per-ray results of the tracer
  double *const ring = reinterpret_cast<double *>(jur_lds);
  double *const epsr = ring + (size_t)PEN_RING * nfield * RB;
  double *const st_tau = epsr + (size_t)PEN_RINGE * (npair > 0 ? npair : 1) * RB;
  double *const c_rad = st_tau + (nchain > 0 ? nchain : 1);
  double *const c_tau = c_rad + nitem;
  double *const c_pp = c_tau + nitem;             // product of the gases' path transmittances after the previous segment
  double *const tsurf = c_pp + nitem;
  unsigned *const st_br = reinterpret_cast<unsigned *>(tsurf + RB);
  unsigned *const st_ix = st_br + (nchain > 0 ? nchain : 1);     // [chain][4]: curve positions (ia, ib packed in [0], [1] without quads)
  int *const npr = reinterpret_cast<int *>(st_ix + 4 * (nchain > 0 ? nchain : 1));
  int const tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  long const ray0 = (long)blockIdx.x * RB;                         // first slot of this workgroup
  int const nray = (int)((c.n - ray0 < RB) ? c.n - ray0 : RB);    // rays it really has

  for (int i = tid; i < nchain; i += blockDim.x) { st_tau[i] = 1.0; st_br[i] = 0; st_ix[4 * i] = st_ix[4 * i + 1] = st_ix[4 * i + 2] = st_ix[4 * i + 3] = 0; }
  for (int i = tid; i < nitem; i += blockDim.x) { c_rad[i] = 0.0; c_tau[i] = 1.0; c_pp[i] = 1.0; }
  for (int i = tid; i < RB; i += blockDim.x) { npr[i] = (i < nray) ? 0 : 1; tsurf[i] = -999; }   // 1: through, no points
  if (tid == 0) {
    ctl.cnt_trace = 0; ctl.done = 0;
    for (int i = 0; i < PEN_MAXE; i++) ctl.cnt_ega[i] = 0;
    for (int i = 0; i < PEN_MAXC; i++) ctl.cnt_comb[i] = 0;
    sl_lo = 0x7fffffff; sl_hi = -1;
  }
  __syncthreads();
  jur_view_t vt = v;                            // the tracer's view of the atmosphere
  if (atm_cap > 0) {
    if (tid < nray) {                           // do all rays of the workgroup use one slice?
      double const time = c.geom[0][c.first + ray0 + tid];
      int const a0 = slice_start(v.atm_time, v.atm_np, time);
      atomicMin(&sl_lo, a0);
      atomicMax(&sl_hi, (v.atm_time[a0] == time) ? a0 : 0x7ffffffe);   // a time stamp without a profile: no copy
    }
    __syncthreads();
    int const a0 = sl_lo;
    if (a0 == sl_hi) {
      // its extent as locate_atm forms it (its second search, jr_common.h:141-152; time stamps are sorted when
      // atm_sorted, otherwise no copy is made): the points that share the first one's time stamp -- and the last
      // point of the atmosphere too when that one alone follows them
      int n = 0;
      if (v.atm_sorted) {
        double const t0 = v.atm_time[a0];
        int lo = a0, hi = v.atm_np - 1;
        while (hi > lo + 1) {
          int const i = (lo + hi) / 2;
          if (v.atm_time[i] > t0) hi = i; else lo = i;
        }
        n = ((hi == v.atm_np - 1) ? v.atm_np : hi) - a0;
      }
      if (n >= 2 && n <= atm_cap) {
        int const nrow = 7 + ng + v.nw;
        double *const slab = reinterpret_cast<double *>(jur_lds) + pen_lds_doubles(nd, ng, v.nw, RB);
        double const *const rows[7] = {v.atm_time, v.atm_z, v.atm_lon, v.atm_lat, v.atm_p, v.atm_t, v.atm_pslope};
        for (int i = tid; i < nrow * n; i += blockDim.x) {
          int const row = i / n, k = i - row * n;
          double x;
          if (row < 7) x = rows[row][a0 + k];
          else if (row < 7 + ng) x = v.atm_q[(size_t)(row - 7) * v.atm_np + a0 + k];
          else x = v.atm_k[(size_t)(row - 7 - ng) * v.atm_np + a0 + k];
          slab[(size_t)row * n + k] = x;
        }
        vt.atm_np = n;
        vt.atm_time = slab; vt.atm_z = slab + n; vt.atm_lon = slab + 2 * n; vt.atm_lat = slab + 3 * n;
        vt.atm_p = slab + 4 * n; vt.atm_t = slab + 5 * n; vt.atm_pslope = slab + 6 * n;
        vt.atm_q = slab + 7 * (size_t)n; vt.atm_k = slab + (7 + (size_t)ng) * n;
        __syncthreads();                          // (uniform branch: every thread of the workgroup is here)
      }
    }
  }

  if (wave == 0) {
    // ---- tracer ----  (QUAD: four lanes per ray, RB <= 16)
    constexpr int SH = QUAD ? 2 : 0;
    int const slot = lane >> SH;
    if (slot < nray) {
      long const ray = c.first + ray0 + slot;
      LosRing L{ring, &ctl, npr, tsurf, nfield, RB, slot, NC, SH, 0ull};
      TraceResult const t = trace_ray<LosRing, QUAD ? 4 : 1>(vt, AtmGlobal{vt}, c.geom[0][ray], c.geom[1][ray], c.geom[2][ray],
                                                     c.geom[3][ray], c.geom[4][ray], c.geom[5][ray], c.geom[6][ray], L, tr_sh,
                                                     c.status);
      if ((lane & ((1 << SH) - 1)) == 0) {
        if (c.np_out) c.np_out[ray] = t.np;
        c.tp[0][ray] = t.tpz;
        c.tp[1][ray] = t.tplon;
        c.tp[2][ray] = t.tplat;
        tsurf[slot] = t.tsurf;
        st_rel(&npr[slot], t.np + 1);        // also the rays that never entered the atmosphere or ran into NLOS
      }
    }
    if (lane == 0) {                         // every ray is through: its point count governs from here on
      int m = 0;
      for (int i = 0; i < nray; i++) m = max(m, ld_acq(&npr[i]) - 1);
      st_rel(&ctl.cnt_trace, m);
      st_rel(&ctl.done, 1);
    }
  } else if (wave <= NE) {
    // ---- emissivity growth: one chain per (ray, channel, gas); with QUAD (sorted tables) a quad of lanes per
    // chain, one corner curve each ----
    constexpr int CS = (QUAD && WARM) ? 2 : 0;                  // lanes per chain = 1 << CS
    int const w = wave - 1, nl = (NE * 64) >> CS, me = (w * 64 + lane) >> CS;
    PairDesc<false> D{v.lvl, v.crv, nullptr, 0u, 0u, 0u, 0u};
    for (int ip = 0;; ++ip) {
      int const cnt = wait_point(&ctl, ip);
      if (cnt <= ip) break;
      if (ip >= PEN_RINGE)
        while (min_cnt(ctl.cnt_comb, NC) + PEN_RINGE <= ip) __builtin_amdgcn_s_sleep(2);
      double const *const slot = ring + (size_t)(ip & (PEN_RING - 1)) * nfield * RB;
      double *const eslot = epsr + (size_t)(ip & (PEN_RINGE - 1)) * npair * RB;
      for (int e = me; e < nchain; e += nl) {
        int const pr = e / RB, r = e - pr * RB, d = pr / ng, g = pr - d * ng;
        int const n1 = ld_acq(&npr[r]);
        if (n1 ? (ip >= n1 - 1) : (ip >= cnt)) continue;          // this ray has no such point
        jur_int2 const pd = v.pair[g * nd + d];
        if (pd.a < 2) continue;                                    // no table: the combine role knows
        D.l0 = (unsigned)pd.b;
        D.ueb = v.ue + v.pair_e0[g * nd + d];
        D.recb = v.fast_arith ? static_cast<void const *>(v.rec + v.pair_e0[g * nd + d]) : nullptr;
        double const p = slot[JUR_F_P * RB + r], t = slot[JUR_F_T * RB + r], u = slot[(JUR_F_K + v.nw + g) * RB + r];
        double const tau_path = st_tau[e];
        double tau_new;                                            // the gas's path transmittance after this segment
        if constexpr (WARM && QUAD) {
          unsigned br = st_br[e], ix = st_ix[4 * e + (lane & 3)];
          if (v.fast_arith) tau_new = ega_eps_warm_quad<true>(v, pd, D, tau_path, t, u, p, br, ix);
          else tau_new = tau_path * ega_eps_warm_quad<false>(v, pd, D, tau_path, t, u, p, br, ix);
          st_br[e] = br; st_ix[4 * e + (lane & 3)] = ix;
        } else if constexpr (WARM) {
          unsigned br = st_br[e], ia = st_ix[4 * e], ib = st_ix[4 * e + 1];
          if (v.fast_arith) tau_new = ega_eps_warm<false, true, true>(v, pd, D, tau_path, t, u, p, br, ia, ib);
          else tau_new = tau_path * ega_eps_warm<false, false>(v, pd, D, tau_path, t, u, p, br, ia, ib);
          st_br[e] = br; st_ix[4 * e] = ia; st_ix[4 * e + 1] = ib;
        } else tau_new = tau_path * ega_eps_exact<false>(v, pd, D, tau_path, t, u, p);
        st_tau[e] = tau_new;
        eslot[pr * RB + r] = tau_new;
      }
      if (first_active_lane()) st_rel(&ctl.cnt_ega[w], ip + 1);
    }
  } else {
    // ---- combine: one lane per (ray, channel) ----
    int const w = wave - 1 - NE, nl = NC * 64, me = w * 64 + lane;
    int const f_u = JUR_F_K + v.nw;
    Exp2Global const e2t;
    for (int ip = 0;; ++ip) {
      int const cnt = wait_point(&ctl, ip);
      if (cnt <= ip) break;
      while (min_cnt(ctl.cnt_ega, NE) <= ip) __builtin_amdgcn_s_sleep(2);
      double const *const slot = ring + (size_t)(ip & (PEN_RING - 1)) * nfield * RB;
      double const *const eslot = epsr + (size_t)(ip & (PEN_RINGE - 1)) * npair * RB;
      for (int i = me; i < nitem; i += nl) {
        int const d = i / RB, r = i - d * RB;
        int const n1 = ld_acq(&npr[r]);
        if (n1 ? (ip >= n1 - 1) : (ip >= cnt)) continue;
        jur_chan_t const ch = v.chan[d];
        auto L = [&](int field) { return slot[field * RB + r]; };
        double const p = L(JUR_F_P), t = L(JUR_F_T), ds = L(JUR_F_DS);
        double beta_ds = (v.atm_k_zero ? 0.0 : L(JUR_F_K + ch.window)) * ds;   // (the tracer role put no extinction into the ring)
        if ((v.fourbit & 8) && ch.co2_on) beta_ds += ctm_co2(ch, p, t, L(f_u + v.ig_co2));
        double const rt = rcp_t(t);
        if ((v.fourbit & 4) && ch.h2o_on) beta_ds += ctm_h2o(e2t, ch, p, t, rt, L(JUR_F_QH2O), L(f_u + v.ig_h2o));
        if ((v.fourbit & 2) && ch.n2_on) beta_ds += ctm_n2(e2t, ch, p, t, rt) * ds;
        if ((v.fourbit & 1) && ch.o2_on) beta_ds += ctm_o2(e2t, ch, p, t, rt) * ds;
        double pcur = 1.0;
        for (int g = 0; g < ng; g++)                       // jr_common.h:272-278
          if (v.pair[g * nd + d].a >= 2) pcur *= eslot[(d * ng + g) * RB + r];
        double const tau_gas = segment_tau_gas(pcur, c_pp[i]);
        c_pp[i] = pcur;
        double rad = c_rad[i], tau = c_tau[i];
        new_obs_step(e2t, tau_gas, beta_ds, planck_src(v.sr + (size_t)d * TBLNS, t), rad, tau);
        c_rad[i] = rad;
        c_tau[i] = tau;
      }
      if (first_active_lane()) st_rel(&ctl.cnt_comb[w], ip + 1);
    }
    for (int i = me; i < nitem; i += nl) {                 // every ray is through (done was seen): epilogue
      int const d = i / RB, r = i - d * RB;
      if (r >= nray) continue;
      size_t const oidx = (size_t)(c.first + ray0 + r) * nd + d;
      bool const masked = !isfinite(c.rad[oidx]);
      double rad = c_rad[i];
      double const tau = c_tau[i];
      ray_epilogue(v.sr + (size_t)d * TBLNS, v.chan[d].nu, tsurf[r], v.write_bbt, rad, tau);
      if (masked) rad = __builtin_nan("");
      c.rad[oidx] = rad;
      c.tau[oidx] = tau;
    }
  }
}

// ---------------------------------------------------------------------------------------
// Curtis-Godson means along the path (curtis_godson, jr_common.h:455-473; upstream compiles it only
// with -DCURTIS_GODSON for FORMOD=1 and never consumes the result): per gas, the inclusive prefix
// sums over the LOS points of u p, u T and u, then cgp = S(u p)/S(u), cgt = S(u T)/S(u), cgu = S(u).
// One wavefront per (ray, gas) pencil, lanes = LOS points: the along-path prefix is a wave scan
// (shuffles), carried from one 64-point chunk to the next.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_inclusive_scan(double x, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    double const y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  return x;
}

__global__ __launch_bounds__(256) void jur_cg_kernel(jur_view_t v, jur_chunk_t c, double *__restrict__ cgp,
                                                     double *__restrict__ cgt, double *__restrict__ cgu) {
  int const lane = threadIdx.x & 63;
  long const wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;   // (slot, gas) pencil
  int const ng = v.ng;
  if (wave >= (long)c.n * ng) return;
  int const r = (int)(wave / ng), g = (int)(wave - (long)r * ng);
  long const ray = c.order ? (long)c.order[r] : c.first + r;
  int const nfield = JUR_F_K + v.nw + ng;
  size_t const R = (size_t)nfield * 64;                              // doubles from one LOS point of a ray to the next
  double const *const tile = c.los + (size_t)(r >> 6) * los_tile_doubles(nfield) + (r & 63);
  double const *const lp = tile + JUR_F_P * 64, *const lt = tile + JUR_F_T * 64,
               *const lu = tile + (size_t)(JUR_F_K + v.nw + g) * 64;
  int const np = c.np[r];
  size_t const out = ((size_t)ray * ng + g) * NLOS;
  double cp = 0, ct = 0, cu = 0;                                         // carry of the previous chunks
  for (int base = 0; base < NLOS; base += 64) {
    int const ip = base + lane;
    double a = 0, b = 0, w = 0;
    if (ip < np) {
      double const u = lu[(size_t)ip * R];
      a = u * lp[(size_t)ip * R];
      b = u * lt[(size_t)ip * R];
      w = u;
    }
    a = wave_inclusive_scan(a, lane) + cp;
    b = wave_inclusive_scan(b, lane) + ct;
    w = wave_inclusive_scan(w, lane) + cu;
    cp = __shfl(a, 63, 64); ct = __shfl(b, 63, 64); cu = __shfl(w, 63, 64);
    if (ip < np) { cgp[out + ip] = a / w; cgt[out + ip] = b / w; cgu[out + ip] = w; }
    else if (ip < NLOS) { cgp[out + ip] = 0; cgt[out + ip] = 0; cgu[out + ip] = 0; }   // NLOS is not a multiple of 64
  }
}

// ---------------------------------------------------------------------------------------
// ray ordering key: altitude of the straight line's closest approach to the Earth's centre;
// optionally grouped by the atmosphere slice the ray uses (neighbouring lanes then walk through
// the same profile, i.e. the same table brackets)
// ---------------------------------------------------------------------------------------
// Bracket records of the emissivity curves, once per model: record i holds entries i and i + 1 and the slopes of
// [entry i, entry i+1] in both directions, formed from the fp32 entries with fp64 differences and IEEE divisions.  The
// last entry of a curve pairs with the first of the next one; the look-up never reads that record (its bracket index
// ends at nu - 2).
__global__ __launch_bounds__(256) void jur_records_kernel(long long n, jur_ue_t const *__restrict__ ue, jur_rec_t *__restrict__ rec) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    double const du = (double)ue[i + 1].u - (double)ue[i].u, de = (double)ue[i + 1].eps - (double)ue[i].eps;
    rec[i] = jur_rec_t{ue[i].u, ue[i].eps, ue[i + 1].u, ue[i + 1].eps, du / de, de / du};
  }
}

// Difference quotients of the batched Jacobian (kernel(), jurassic.c:853-855): the radiances of the n perturbed copies
// of the nr rays stand behind the unperturbed ones, rad[(e + 1) * nr + i][id]; dense rows q = i * nd + id, columns e:
// kq[q][e] = (y1 - y0) / h[e].  One lane per element, columns fastest.
__global__ __launch_bounds__(256) void jur_kquot_kernel(long nq, long n, long nrnd, double const *__restrict__ rad,
                                                        double const *__restrict__ h, double *__restrict__ kq) {
  long const t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nq * n) return;
  long const q = t / n, e = t - q * n;
  kq[t] = (rad[(e + 1) * nrnd + q] - rad[q]) / h[e];
}

// longest path of every tile of 64 ray slots (what the tile needs of the transmittance workspace), one wavefront per tile
__global__ __launch_bounds__(256) void jur_tilemax_kernel(int n, int const *__restrict__ np, int *__restrict__ tile_np) {
  int const r = blockIdx.x * blockDim.x + threadIdx.x;
  int m = r < n ? np[r] : 0;
  for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0 && (r >> 6) < (n + 63) / 64) tile_np[r >> 6] = m;
}

__global__ __launch_bounds__(256) void jur_raykey_kernel(long nr, long ld, double const *__restrict__ geom,
                                                         double const *__restrict__ atm_time, int atm_np, int by_profile,
                                                         unsigned long long *__restrict__ key, int *__restrict__ id) {
  long const r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nr) return;
  double xo[3], xv[3], e[3];
  geo2cart(geom[1 * ld + r], geom[2 * ld + r], geom[3 * ld + r], xo);      // field k of ray r: geom[k * ld + r]
  geo2cart(geom[4 * ld + r], geom[5 * ld + r], geom[6 * ld + r], xv);
  for (int i = 0; i < 3; i++) e[i] = xv[i] - xo[i];
  double const n = norm3(e);
  double h = norm3(xo) - JUR_RE;
  if (n > 0) {
    double s = 0;
    for (int i = 0; i < 3; i++) s -= xo[i] * e[i] / n;
    if (s > 0) h = sqrt(fmax(xo[0] * xo[0] + xo[1] * xo[1] + xo[2] * xo[2] - s * s, 0.)) - JUR_RE;
  }
  unsigned const fb = __float_as_uint((float)h);
  unsigned const ord = fb ^ ((fb >> 31) ? 0xffffffffu : 0x80000000u);   // unsigned order == float order
  unsigned long long slice = 0;
  if (by_profile) {  // first point of the profile slice with this ray's time stamp (jr_common.h:130-140)
    double const time = geom[r];
    int lo = 0, hi = atm_np - 1;
    while (hi > lo + 1) {
      int const i = (lo + hi) / 2;
      if (atm_time[i] < time) lo = i; else hi = i;
    }
    slice = (unsigned long long)((0 == lo) ? lo : hi);
  }
  key[r] = (slice << 32) | ord;
  id[r] = (int)r;
}

// One key per block of 256 consecutive slots of the sorted launch, a wavefront per block: the tangent-altitude bits (the
// low word of the sorted key) of the block's LOWEST ray, the one with the longest path.  Within a profile the slots
// ascend in tangent altitude and that is the block's first slot; a block that straddles two profiles begins with the
// highest rays of one and holds the lowest of the next, which cost the most (keyed by its first slot it would start
// last and be the launch's tail: tools/dispatch_order_model.py).
__global__ __launch_bounds__(256) void jur_blockkey_kernel(long nr, int nblk, unsigned long long const *__restrict__ sorted_key,
                                                           unsigned *__restrict__ key, int *__restrict__ id) {
  int const b = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = (int)(threadIdx.x & 63);
  if (b >= nblk) return;                               // (whole wavefronts: b is uniform)
  unsigned m = 0xffffffffu;
  for (int k = 0; k < 4; k++) {
    long const r = (long)b * 256 + k * 64 + lane;
    if (r < nr) m = min(m, (unsigned)sorted_key[r]);
  }
  for (int o = 32; o > 0; o >>= 1) m = min(m, (unsigned)__shfl_xor((int)m, o));
  if (lane == 0) { key[b] = m; id[b] = b; }
}

// ---------------------------------------------------------------------------------------
// field-of-view convolution on device arrays (formod_fov, jurassic.c:214-258): for callers that keep the
// radiances in HBM.  One lane per (ray, channel); the neighbours' profile is gathered per lane, the weights are
// walked in the reference's order with its arithmetic (jur_fov.c is the host twin, bit-identical).
// rad0 / tau0: the forward model's results [nr][nd]; rad / tau: the convolved ones [nr][ld].
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jur_fov_kernel(long nr, int nd, double const *__restrict__ time, double const *__restrict__ vpz,
                                                      double const *__restrict__ rad0, double const *__restrict__ tau0,
                                                      double *__restrict__ rad, double *__restrict__ tau, long ld, int n,
                                                      double const *__restrict__ dz, double const *__restrict__ w,
                                                      int *__restrict__ status) {
  long const i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nr * nd) return;
  long const ir = i / nd;
  int const id = (int)(i - ir * nd);
  double z[2 * JUR_NFOV + 1];
  long src[2 * JUR_NFOV + 1];
  int nz = 0;
  long const lo = ir - JUR_NFOV > 0 ? ir - JUR_NFOV : 0, hi = ir + 1 + JUR_NFOV < nr ? ir + 1 + JUR_NFOV : nr;
  for (long ir2 = lo; ir2 < hi; ir2++)
    if (time[ir2] == time[ir]) { z[nz] = vpz[ir2]; src[nz] = ir2; nz++; }
  if (nz < 2) { atomicOr(status, 2); return; }          // "Cannot apply FOV convolution!" upstream
  double r = 0, t = 0, wsum = 0;
  for (int k = 0; k < n; k++) {
    double const zfov = vpz[ir] + dz[k];
    int const idx = locate_axis(z, nz, zfov);
    double const r0 = rad0[src[idx] * nd + id], r1 = rad0[src[idx + 1] * nd + id];
    double const t0 = tau0[src[idx] * nd + id], t1 = tau0[src[idx + 1] * nd + id];
    r += w[k] * (r0 + (zfov - z[idx]) * (r1 - r0) / (z[idx + 1] - z[idx]));
    t += w[k] * (t0 + (zfov - z[idx]) * (t1 - t0) / (z[idx + 1] - z[idx]));
    wsum += w[k];
  }
  rad[ir * ld + id] = r / wsum;
  tau[ir * ld + id] = t / wsum;
}

// ---------------------------------------------------------------------------------------
// atmosphere regridding (intpol_atm, jurassic.c:675-804): the step in front of the path for atmospheres that
// are not one profile.  One lane per destination point; ip = 1 one profile, 2 the nearest two profiles of a
// track, 3 the distance-weighted mean of a point cloud.  The Cartesian positions of source and destination points
// come from the host (they are what upstream caches), the kernel does the searches and the interpolation.
// src rows: z, lon, lat, p, T, q[ng], k[nw], each [ns]; out rows: p, T, q[ng], k[nw], each [nd_].
// ---------------------------------------------------------------------------------------
struct IntpolArgs {
  int ip, ng, nw, ns, nd_, nx;
  double cx, cz;
  double const *src;        // [5 + ng + nw][ns]
  double const *x1;         // ip 2: [nx][3] profile positions; ip 3: [ns][3] point positions
  int const *idx, *nz;      // ip 2: first point and length of every profile
  double const *dst;        // [3][nd_]: z, lon, lat of the destination points
  double const *x0;         // [nd_][3] their positions
  double *out;              // [2 + ng + nw][nd_]
};

__device__ __forceinline__ double eip_dev(double x0, double y0, double x1, double y1, double x) {
  if ((y0 > 0) && (y1 > 0)) return y0 * exp(log(y1 / y0) / (x1 - x0) * (x - x0));
  return lip(x0, y0, x1, y1, x);
}

// intpol_atm_1d on source points [i0, i0 + n): row r of the source interpolated to z0
__device__ __forceinline__ double ip1d(IntpolArgs const &a, int ipt, int row, double z0) {
  double const *const z = a.src, *const y = a.src + (size_t)row * a.ns;
  return (row == 3) ? eip_dev(z[ipt], y[ipt], z[ipt + 1], y[ipt + 1], z0) : lip(z[ipt], y[ipt], z[ipt + 1], y[ipt + 1], z0);
}

__global__ __launch_bounds__(128) void jur_intpol_kernel(IntpolArgs a) {
  int const id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= a.nd_) return;
  int const nrow = 2 + a.ng + a.nw;                       // p, T, q[], k[]: source rows 3 ..
  double const z0 = a.dst[id], lat0 = a.dst[2 * (size_t)a.nd_ + id];
  double const x0[3] = {a.x0[3 * (size_t)id], a.x0[3 * (size_t)id + 1], a.x0[3 * (size_t)id + 2]};
  auto OUT = [&](int r) -> double & { return a.out[(size_t)r * a.nd_ + id]; };
  if (a.ip == 1) {
    int const ipt = locate_axis(a.src, a.ns, z0);
    for (int r = 0; r < nrow; r++) OUT(r) = ip1d(a, ipt, 3 + r, z0);
  } else if (a.ip == 2) {
    double dhmin0 = 1e99, dhmin1 = 1e99;
    int ix0 = 0, ix1 = 0;
    double const *const lat = a.src + 2 * (size_t)a.ns;
    for (int ix = 0; ix < a.nx; ix++)
      if (fabs(lat0 - lat[a.idx[ix]]) <= 10) {
        double const *const x1 = a.x1 + 3 * (size_t)ix;
        double const dh = (x0[0] - x1[0]) * (x0[0] - x1[0]) + (x0[1] - x1[1]) * (x0[1] - x1[1]) + (x0[2] - x1[2]) * (x0[2] - x1[2]);
        if (dh <= dhmin0) { dhmin1 = dhmin0; ix1 = ix0; dhmin0 = dh; ix0 = ix; }
        else if (dh <= dhmin1) { dhmin1 = dh; ix1 = ix; }
      }
    int const i0 = a.idx[ix0] + locate_axis(a.src + a.idx[ix0], a.nz[ix0], z0);
    int const i1 = a.idx[ix1] + locate_axis(a.src + a.idx[ix1], a.nz[ix1], z0);
    double const *const xa = a.x1 + 3 * (size_t)ix0, *const xb = a.x1 + 3 * (size_t)ix1;
    double const x2 = (xa[0] - xb[0]) * (xa[0] - xb[0]) + (xa[1] - xb[1]) * (xa[1] - xb[1]) + (xa[2] - xb[2]) * (xa[2] - xb[2]);
    double const x = sqrt(x2);
    double const r0 = (dhmin0 - dhmin1 + x2) / (2 * x);
    double const r1 = x - r0;
    double r;
    if (r0 <= 0) r = 0;
    else r = (r1 <= 0) ? 1 : r0 / (r0 + r1);
    for (int k = 0; k < nrow; k++) OUT(k) = (1 - r) * ip1d(a, i0, 3 + k, z0) + r * ip1d(a, i1, 3 + k, z0);
  } else {
    double const rm2 = a.cx * a.cx;
    double wsum = 0;
    for (int r = 0; r < nrow; r++) OUT(r) = 0;
    double const *const lat = a.src + 2 * (size_t)a.ns;
    for (int ipt = 0; ipt < a.ns; ipt++) {
      double const dz = fabs(a.src[ipt] - z0);
      if (dz >= a.cz) continue;
      if (fabs(lat[ipt] - lat0) * 111.13 >= a.cx) continue;
      double const *const x1 = a.x1 + 3 * (size_t)ipt;
      double const dx2 = (x0[0] - x1[0]) * (x0[0] - x1[0]) + (x0[1] - x1[1]) * (x0[1] - x1[1]) + (x0[2] - x1[2]) * (x0[2] - x1[2]);
      if (dx2 >= rm2) continue;
      double const w = (1 - dz / a.cz) * (rm2 - dx2) / (rm2 + dx2);
      wsum += w;
      for (int r = 0; r < nrow; r++) OUT(r) += w * a.src[(size_t)(3 + r) * a.ns + ipt];
    }
    if (wsum >= 1e-6) for (int r = 0; r < nrow; r++) OUT(r) /= wsum;
    else for (int r = 0; r < nrow; r++) OUT(r) = __builtin_nan("");
  }
}

// ---------------------------------------------------------------------------------------
// known-answer hooks (tests): the device functions above on arrays of inputs, one element per lane,
// so that each can be compared with its reference counterpart at thresholds and range edges
// (jr_common.h:239 tau < 1e-9, :295 tau_gas > 1e-50, continuum windows :318,345,367,381, extrapolation
// beyond both ends of a curve) without a ray around it.  Not on the product path.
// ---------------------------------------------------------------------------------------
// chain != 0: ONE lane walks the n inputs in order and carries the warm-start state (br, ia, ib) from element
// to element as jur_ega_kernel carries it from segment to segment -- the result of a look-up must not depend on
// where the previous one left the brackets.
template <bool WARM, bool LDS, bool RCPB>
__global__ __launch_bounds__(256) void jur_kat_ega_kernel(jur_view_t v, int g, int d, long n, double const *__restrict__ tau,
                                                          double const *__restrict__ t, double const *__restrict__ u,
                                                          double const *__restrict__ p, int chain, double *__restrict__ out) {
  jur_int2 const pd = v.pair[g * v.nd + d];
  PairDesc<LDS> D{v.lvl, v.crv, v.ue + v.pair_e0[g * v.nd + d], (unsigned)pd.b, 0u, 0u, 0u};
  if constexpr (RCPB) D.recb = v.rec + v.pair_e0[g * v.nd + d];
  if (pd.a >= 2) stage_pair<LDS, RCPB>(v, pd, D);       // uniform branch; stage_pair ends in a barrier
  unsigned br = 0, ia = 0, ib = 0;
  auto one = [&](long i) {
    if constexpr (WARM) out[i] = ega_eps_warm<LDS, RCPB>(v, pd, D, tau[i], t[i], u[i], p[i], br, ia, ib);
    else out[i] = ega_eps_exact<LDS>(v, pd, D, tau[i], t[i], u[i], p[i]);
  };
  if (chain) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
      for (long i = 0; i < n; i++) one(i);
  } else {
    long const i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) one(i);
  }
}

// the Curtis-Godson look-up on arrays of (tau, cgt, cgu, cgp): the new path transmittance (cga_tau_*; the running sums
// and the w == 0 rule belong to the ray, not to the look-up)
template <bool WARM, bool LDS, bool RCPB>
__global__ __launch_bounds__(256) void jur_kat_cga_kernel(jur_view_t v, int g, int d, long n, double const *__restrict__ tau,
                                                          double const *__restrict__ t, double const *__restrict__ u,
                                                          double const *__restrict__ p, int chain, double *__restrict__ out) {
  jur_int2 const pd = v.pair[g * v.nd + d];
  PairDesc<LDS> D{v.lvl, v.crv, v.ue + v.pair_e0[g * v.nd + d], (unsigned)pd.b, 0u, 0u, 0u};
  if constexpr (RCPB) D.recb = v.rec + v.pair_e0[g * v.nd + d];
  if (pd.a >= 2) stage_pair<LDS, RCPB>(v, pd, D);       // uniform branch; stage_pair ends in a barrier
  unsigned br = 0, ia = 0, ib = 0;
  auto one = [&](long i) {
    if constexpr (WARM) out[i] = cga_tau_warm<LDS, RCPB>(pd, D, tau[i], t[i], u[i], p[i], br, ia, ib);
    else out[i] = cga_tau_exact<LDS>(pd, D, tau[i], t[i], u[i], p[i]);
  };
  if (chain) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
      for (long i = 0; i < n; i++) one(i);
  } else {
    long const i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) one(i);
  }
}

// out[0..3][n]: CO2, H2O, N2, O2 continuum terms of channel d as jur_combine_kernel adds them (0 outside a window)
__global__ __launch_bounds__(256) void jur_kat_continua_kernel(jur_view_t v, int d, long n, double const *__restrict__ p,
                                                               double const *__restrict__ t, double const *__restrict__ q,
                                                               double const *__restrict__ u_co2, double const *__restrict__ u_h2o,
                                                               double *__restrict__ out) {
  long const i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  jur_chan_t const ch = v.chan[d];
  out[i] = ch.co2_on ? ctm_co2(ch, p[i], t[i], u_co2[i]) : 0.;
  double const rt = rcp_t(t[i]);
  Exp2Global const e2t;
  out[n + i] = ch.h2o_on ? ctm_h2o(e2t, ch, p[i], t[i], rt, q[i], u_h2o[i]) : 0.;
  out[2 * n + i] = ch.n2_on ? ctm_n2(e2t, ch, p[i], t[i], rt) : 0.;
  out[3 * n + i] = ch.o2_on ? ctm_o2(e2t, ch, p[i], t[i], rt) : 0.;
}

// what == 0: src = source function at t = a[i]; (rad, tau) updated by one segment with tau_gas = b[i], beta_ds = c[i]
// what == 1: epilogue with surface temperature a[i] and brightness conversion if b[i] != 0; src = source at a[i]
__global__ __launch_bounds__(256) void jur_kat_update_kernel(jur_view_t v, int d, long n, int what, double const *__restrict__ a,
                                                             double const *__restrict__ b, double const *__restrict__ c,
                                                             double *__restrict__ rad, double *__restrict__ tau,
                                                             double *__restrict__ src) {
  long const i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double const *const sr = v.sr + (size_t)d * TBLNS;
  double r = rad[i], tt = tau[i];
  src[i] = planck_src(sr, a[i]);
  if (what == 0) new_obs_step(Exp2Global(), b[i], c[i], src[i], r, tt);
  else ray_epilogue(sr, v.chan[d].nu, a[i], b[i] != 0., r, tt);
  rad[i] = r;
  tau[i] = tt;
}

// The LOS records of a traced chunk as the tracer left them in the workspace, [tile][point][field][64], gathered to
// los[ray][field][NLOS] and tsurf[ray] by ray id: one lane per (slot, point), plain loads and stores.  Points from
// np[slot] on read nothing and come back 0; so does the q_H2O row when the tracer never writes it (v.ig_h2o < 0).
__global__ __launch_bounds__(256) void jur_kat_los_kernel(jur_view_t v, jur_chunk_t c, double *__restrict__ los,
                                                          double *__restrict__ tsurf) {
  long const i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)c.n * NLOS) return;
  int const r = (int)(i / NLOS), ip = (int)(i - (long)r * NLOS);
  long const ray = c.order ? (long)c.order[r] : c.first + r;
  int const nfield = JUR_F_K + v.nw + v.ng;
  int const np = c.np[r] < NLOS ? c.np[r] : NLOS;
  double const *const src = c.los + (size_t)(r >> 6) * los_tile_doubles(nfield) + (size_t)ip * nfield * 64 + (r & 63);
  double *const dst = los + (size_t)ray * nfield * NLOS + ip;
  for (int f = 0; f < nfield; f++) {
    // (an atmosphere without extinction: the tracer leaves the extinction fields alone, and they are the +0.0 it would write)
    bool const written = ip < np && !(f == JUR_F_QH2O && v.ig_h2o < 0) && !(v.atm_k_zero && f >= JUR_F_K && f < JUR_F_K + v.nw);
    dst[(size_t)f * NLOS] = written ? src[(size_t)f * 64] : 0.;
  }
  if (ip == 0) tsurf[ray] = c.tsurf[r];
}

// ---- block Jacobian of a scene (jur_kernel_scene_host): streaming copies and one division per element ----------------
// largest i in [lo, hi) with a[i] + bias(i) <= x, for a non-decreasing a[] with a[lo] + bias(lo) <= x
template <bool PlusIndex>
__device__ inline long scene_find(long const *__restrict__ a, long lo, long hi, long x) {
  while (hi - lo > 1) {
    long const mid = lo + ((hi - lo) >> 1);
    if (a[mid] + (PlusIndex ? mid : 0) <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// The stacked atmosphere, one lane per (copy, point): copy 0 is the base atmosphere as it stands, copy j >= 1 the points
// [first, first + len) of one slice under ONE time stamp tmax + j * span, with the value of row prow at base point pip
// raised by the reference's step (jurassic.c:831-837), formed here from the base value with the host's operations
// (kernel_ld in jur_model.c) and kept in h[j].  Lanes of a wavefront read and write consecutive points of every row.
__global__ __launch_bounds__(256) void jur_scene_stack_kernel(jur_scene_stack_t a) {
  long const t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.nt) return;
  long const j = scene_find<false>(a.off, 0, a.ncopy, t);
  long const src = a.first[j] + (t - a.off[j]);
  int const prow = a.prow[j];
  bool const raised = prow >= 0 && src == a.pip[j];
  for (int row = 0; row < a.nrow; row++) {
    double x = a.base[(long)row * a.np0 + src];
    if (row == 0 && j > 0) x = a.tmax + (double)j * a.span;
    if (raised && row == prow) {
      double hh;
      if (row == 4) hh = fmax(fabs(0.01 * x), 1e-7);
      else if (row == 5) hh = 1;
      else if (row < 6 + a.ng) hh = fmax(fabs(0.01 * x), 1e-15);
      else hh = 1e-4;
      a.h[j] = hh;
      x = x + hh;
    }
    a.rows[(long)row * a.nt + t] = x;
  }
}

// ---- hydrostatic balance of the slices of a scene (jur_model_set_scene_hydz) ------------------------------------------
// One wavefront per segment [at, at + len) of the rows: hydrostatic_1d_h2o (jr_common.h:713-761) on that profile alone, the
// host rule of jur_scene_hydrostatic operand for operand (this file is compiled without contraction).
//  (a) the reference parcel: every lane keeps the first minimum of |z - hydz| over its points i = lane, lane + 64, ...
//      (strict <, ascending i), then a fixed xor tree over (distance, index) in which the lower index wins a tie: the
//      first minimal index of the segment, whatever the lanes' order -- the host's `if (dz < dzmin)` scan.
//  (b) layer l joins the points l and l + 1.  From the parcel upwards it is integrated from l to l + 1, below it from
//      l + 1 to l, as the reference's two loops do.  Lane j of a chunk takes the j-th layer above the parcel and the j-th
//      below it and forms f = exp(-1000 * mean * dz) with the 20 terms of the mean ascending; the latitude's two sines
//      and the altitude-free part of gravity() are formed once per segment.
//  (c) the factors lie in LDS, 64 of either direction at a time.  Lane 0 runs the upward chain p[ip] = p[ip - 1] * f and
//      lane 1 the downward one, each a sequential product in the reference's order (a scan would round differently), and
//      leave the pressures in LDS; all lanes then store them.
// p of the parcel is never written and no f depends on a pressure, so a second balance of a balanced segment gives the
// same bits.  No atomics; a double depends on its own segment's inputs alone.
__device__ inline double hydro_factor(jur_scene_hydro_t const &a, long base, int from, int to, double g0) {
  double const mmair = 28.96456e-3, mmh2o = 18.0153e-3;
  double const zf = a.z[base + from], zt = a.z[base + to], tf = a.t[base + from], tt = a.t[base + to];
  double const qf = a.q ? a.q[base + from] : 0., qt = a.q ? a.q[base + to] : 0.;
  double mean = 0., e = 0.;
  for (int i = 0; i < 20; i++) {
    double const x = (double)i;
    double const zz = zf + (x - 0.0) * (zt - zf) / (19.0 - 0.0);
    double const grav = g0 - 3.086e-3 * zz;
    if (a.q) e = qf + (x - 0.0) * (qt - qf) / (19.0 - 0.0);
    double const temp = tf + (x - 0.0) * (tt - tf) / (19.0 - 0.0);
    mean += (e * mmh2o + (1 - e) * mmair) * grav / (JUR_MOLAR_GAS * temp * 20);
  }
  return exp(-1000 * mean * (zt - zf));
}

__global__ __launch_bounds__(64) void jur_scene_hydro_kernel(jur_scene_hydro_t a) {
  __shared__ double up[64], down[64];
  long const seg = blockIdx.x;
  int const lane = threadIdx.x, n = a.len[seg];
  if (n < 2) return;
  long const base = a.at[seg];
  // (a)
  double best = 1e99;
  int ipref = 0x7fffffff;
  for (int i = lane; i < n; i += 64) {
    double const dz = fabs(a.z[base + i] - a.hydz);
    if (dz < best) { best = dz; ipref = i; }
  }
  for (int m = 1; m < 64; m <<= 1) {
    double const ob = __shfl_xor(best, m, 64);
    int const oi = __shfl_xor(ipref, m, 64);
    if (ob < best || (ob == best && oi < ipref)) { best = ob; ipref = oi; }
  }
  if (ipref == 0x7fffffff) ipref = 0;               // (no distance below 1e99: the host's initial value)
  // (b)
  double const deg2rad = M_PI / 180., lat = a.lat[base + ipref];
  double const sx = sin(lat * deg2rad), sy = sin(2 * lat * deg2rad);
  double const g0 = 9.780318 * (1. + 0.0053024 * sx * sx - 5.8e-6 * sy * sy);
  int const nup = n - 1 - ipref, ndown = ipref;     // layers above and below the parcel
  double pu = a.p[base + ipref], pd = pu;           // (lanes 0 and 1 carry the chains)
  for (int c = 0; c < nup || c < ndown; c += 64) {
    int const j = c + lane;
    if (j < nup) up[lane] = hydro_factor(a, base, ipref + j, ipref + j + 1, g0);
    if (j < ndown) down[lane] = hydro_factor(a, base, ipref - j, ipref - j - 1, g0);
    __syncthreads();
    // (c)
    if (lane < 2) {
      double *const f = lane ? down : up;
      int const left = (lane ? ndown : nup) - c, m = left < 64 ? left : 64;
      double pr = lane ? pd : pu;
      for (int i = 0; i < m; i++) { pr = pr * f[i]; f[i] = pr; }
      if (lane) pd = pr; else pu = pr;
    }
    __syncthreads();
    if (j < nup) a.p[base + ipref + j + 1] = up[lane];
    if (j < ndown) a.p[base + ipref - j - 1] = down[lane];
    __syncthreads();
  }
}

// slot of ray r in the pass that starts at ray r0
__device__ inline long scene_slot(jur_scene_pass_t const &a, long r) { return (a.rowptr[r] - a.rowptr[a.r0]) + (r - a.r0); }

// Replicated geometry of a pass, one lane per slot: copy 0 of a ray carries the time stamp of its slice's first point in
// the stacked base block (`above`, and with it one point alone, where its slice is a single point), copy e + 1 the time
// stamp of the stacked copy that raises element e of its slice.
__global__ __launch_bounds__(256) void jur_scene_rays_kernel(jur_scene_pass_t a) {
  long const s = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= a.n) return;
  long const r = scene_find<true>(a.rowptr, a.r0, a.r1, s + a.rowptr[a.r0] + a.r0);
  long const e = s - scene_slot(a, r);
  double time;
  if (e == 0) time = a.len[r] >= 2 ? a.atm_time[a.first[r]] : a.above;
  else time = a.atm_time[a.off[a.copy0[r] + e - 1]];
  a.geom[s] = time;
  for (int q = 1; q < 7; q++) a.geom[q * a.n + s] = a.in_geom[q * a.nr + r];
}

// ... and its input radiances (the NaN mask), one lane per (slot, channel)
__global__ __launch_bounds__(256) void jur_scene_mask_kernel(jur_scene_pass_t a) {
  long const t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.n * a.nd) return;
  long const s = t / a.nd, id = t - s * a.nd;
  long const r = scene_find<true>(a.rowptr, a.r0, a.r1, s + a.rowptr[a.r0] + a.r0);
  a.rad[t] = a.in_rad[r * a.nd + id];
}

// Difference quotients of a pass straight into the block layout, one lane per element: block of ray r at
// (rowptr[r] - rowptr[r0]) * nd, [nd][width], entry (id, e) = (rad[copy e + 1][id] - rad[copy 0][id]) / h.
__global__ __launch_bounds__(256) void jur_scene_quot_kernel(jur_scene_pass_t a) {
  long const t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long const base = a.rowptr[a.r0];
  if (t >= (a.rowptr[a.r1] - base) * a.nd) return;
  long const r = scene_find<false>(a.rowptr, a.r0, a.r1, base + t / a.nd);   // the last ray that starts there: the one with columns
  long const w = a.rowptr[r + 1] - a.rowptr[r];
  long const local = t - (a.rowptr[r] - base) * a.nd;
  long const id = local / w, e = local - id * w;
  long const s0 = scene_slot(a, r);
  a.k[t] = (a.rad[(s0 + e + 1) * a.nd + id] - a.rad[s0 * a.nd + id]) / a.h[a.copy0[r] + e];
}

// copy 0 of every ray of a pass into the caller's order, one lane per (ray, channel)
__global__ __launch_bounds__(256) void jur_scene_gather_kernel(jur_scene_pass_t a) {
  long const t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (a.r1 - a.r0) * a.nd) return;
  long const r = a.r0 + t / a.nd, id = t - (r - a.r0) * a.nd;
  long const s0 = scene_slot(a, r);
  a.out_rad[r * a.nd + id] = a.rad[s0 * a.nd + id];
  a.out_tau[r * a.nd + id] = a.fov_tau ? a.fov_tau[t] : a.tau[s0 * a.nd + id];
  if (id == 0) {
    for (int q = 0; q < 3; q++) a.out_tp[q * a.nr + r] = a.tp[q * a.n + s0];
    a.out_np[r] = a.np[s0];
  }
}

// ---- field of view of the scene entries (jur_model_set_fov) ----------------------------------------------------------
// One workgroup per ray of the pass.  Lane 0 gathers the window (the rays of the pass within JUR_NFOV positions that carry
// the ray's time stamp: view-point altitude and first value of each) into LDS; the points of the shape are then taken
// FOV_CH at a time: lane k of a chunk finds the bracket of vpz + dz[k] with locate_axis and leaves idx, zfov - z[idx],
// z[idx + 1] - z[idx] and w[k] in LDS, so that what is staged does not grow with the shape.  The lanes run over the
// ray's contiguous values (copy or trial major, channel inside), 256 at a time, and every neighbour is read as one
// coalesced stretch.  The arithmetic is jur_fov_kernel's, operand for operand and in its order (ascending k, one division
// by the sum of the weights at the end), so that a value is bit for bit what jur_fov_apply makes of the same radiances.
// A shape of more than FOV_CH points is staged again for every 256 values.  No atomics but the status word.
#define FOV_CH 64
__global__ __launch_bounds__(256) void jur_scene_fov_kernel(jur_scene_fov_t a) {
  __shared__ double z[2 * JUR_NFOV + 1], dzl[FOV_CH], dzw[FOV_CH], wk[FOV_CH];
  __shared__ long src[2 * JUR_NFOV + 1];
  __shared__ int ix[FOV_CH], nzs;
  long const r = a.r0 + blockIdx.x;
  int const nd = a.nd, lane = threadIdx.x;
  long const base = a.ntrial > 0 ? 0 : a.rowptr[a.r0];
  if (lane == 0) {
    int nz = 0;
    long const lo = r - JUR_NFOV > a.r0 ? r - JUR_NFOV : a.r0, hi = r + 1 + JUR_NFOV < a.r1 ? r + 1 + JUR_NFOV : a.r1;
    for (long r2 = lo; r2 < hi; r2++)
      if (a.time[r2] == a.time[r]) {
        z[nz] = a.vpz[r2];
        src[nz] = (a.ntrial > 0 ? (r2 - a.r0) * a.ntrial : (a.rowptr[r2] - base) + (r2 - a.r0)) * nd;
        nz++;
      }
    nzs = nz;
  }
  __syncthreads();
  int const nz = nzs;
  if (nz < 2) {                                             // (uniform) "Cannot apply FOV convolution!" upstream
    if (lane == 0) atomicOr(a.status, 2);
    return;
  }
  long const mine = (a.ntrial > 0 ? (r - a.r0) * a.ntrial : (a.rowptr[r] - base) + (r - a.r0)) * nd;
  long const L = (a.ntrial > 0 ? (long)a.ntrial : a.rowptr[r + 1] - a.rowptr[r] + 1) * nd;
  double const vz = a.vpz[r];
  bool const restage = a.n > FOV_CH;
  for (long v0 = 0; v0 < L; v0 += 256) {
    long const v = v0 + lane;
    bool const on = v < L, with_tau = a.tau && v < nd;
    double rr = 0, tt = 0, wsum = 0;
    for (int k0 = 0; k0 < a.n; k0 += FOV_CH) {
      int const nk = a.n - k0 < FOV_CH ? a.n - k0 : FOV_CH;
      if (restage || v0 == 0) {
        __syncthreads();                                    // (the readers of the chunk before)
        if (lane < nk) {
          double const zfov = vz + a.dz[k0 + lane];
          int const idx = locate_axis((double const *)z, nz, zfov);
          ix[lane] = idx; dzl[lane] = zfov - z[idx]; dzw[lane] = z[idx + 1] - z[idx]; wk[lane] = a.w[k0 + lane];
        }
        __syncthreads();
      }
      if (on)
        for (int k = 0; k < nk; k++) {
          int const idx = ix[k];
          double const w = wk[k], dl = dzl[k], dw = dzw[k];
          double const r0 = a.rad[src[idx] + v], r1 = a.rad[src[idx + 1] + v];
          rr += w * (r0 + dl * (r1 - r0) / dw);
          if (with_tau) {
            double const t0 = a.tau[src[idx] + v], t1 = a.tau[src[idx + 1] + v];
            tt += w * (t0 + dl * (t1 - t0) / dw);
          }
          wsum += w;
        }
    }
    if (on) a.rad_f[mine + v] = rr / wsum;
    if (with_tau) a.tau_f[(r - a.r0) * nd + v] = tt / wsum;
  }
}

// ---- normal equations of a scene (jur_normal_scene_host) -------------------------------------------------------------
// first i in [lo, hi) with a[i] >= x (hi if none), for an ascending a[]
__device__ inline long scene_lower(int const *__restrict__ a, long lo, long hi, long x) {
  while (lo < hi) {
    long const mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One workgroup per 16 x 16 tile (ti, tj), tj <= ti, of one slice's A; lane (ty, tx) owns A[16 ti + ty][16 tj + tx] and
// carries its chain of terms weight * K[id][i] * K[id][j] over the slice's rays of the pass, ascending, and their
// channels, ascending: the chain starts from the value the earlier passes left and goes back there, so where a pass
// ends changes no bit.  The measurements (ray, channel) of the sub-range are taken eight at a time: the 32 entries of
// each block row that the tile needs (columns of ti, then of tj) are staged in LDS, one per lane, in one of two buffers
// (one barrier per group: a lane can be no further than one group ahead of the slowest), with the weight (0: not live,
// the term is skipped, so that the NaN row of a masked channel is never multiplied) and y - F.  K_i * K_j is rounded
// first and is the same for (i, j) and (j, i), so the mirror image written for tj < ti equals what a tile (tj, ti) would
// have made, and the two halves of a diagonal tile agree bit for bit.  The tiles of the first tile column (tj == 0) carry
// b of their rows in the lanes tx == 0, tile (0, 0) cost and nlive in lane 0.
__global__ __launch_bounds__(256) void jur_scene_normal_kernel(jur_scene_pass_t a, jur_scene_normal_t n) {
  __shared__ double rows[2][8][32];
  __shared__ double wl[2][8], dl[2][8];
  long const s = scene_find<false>(n.tptr, 0, n.nslice, (long)blockIdx.x);
  long const q0 = scene_lower(n.srays, n.sptr[s], n.sptr[s + 1], a.r0), q1 = scene_lower(n.srays, q0, n.sptr[s + 1], a.r1);
  if (q1 == q0) return;                                   // (uniform: before any barrier)
  long const t = (long)blockIdx.x - n.tptr[s];
  int ti = 0;
  while ((long)(ti + 1) * (ti + 2) / 2 <= t) ti++;
  int const tj = (int)(t - (long)ti * (ti + 1) / 2);
  int const w = (int)(n.wptr[s + 1] - n.wptr[s]), nd = a.nd;
  int const ty = threadIdx.x >> 4, tx = threadIdx.x & 15, i = ti * 16 + ty, j = tj * 16 + tx;
  bool const inside = i < w && j < w, with_b = tj == 0 && tx == 0 && i < w, with_cost = ti == 0 && threadIdx.x == 0;
  double *const As = n.A + n.aptr[s];
  double acc = inside ? As[(long)i * w + j] : 0.;
  double acc_b = with_b ? n.b[n.wptr[s] + i] : 0.;
  double acc_c = with_cost ? n.cost[s] : 0.;
  long count = with_cost ? n.nlive[s] : 0;
  int const lc = threadIdx.x >> 5, lcol = threadIdx.x & 31;
  int const col = lcol < 16 ? ti * 16 + lcol : tj * 16 + lcol - 16;
  long const M = (q1 - q0) * nd, kbase = a.rowptr[a.r0];
  for (long m0 = 0; m0 < M; m0 += 8) {
    int const buf = (int)(m0 >> 3) & 1;
    long const mm = m0 + lc;
    double v = 0., ww = 0., d = 0.;
    if (mm < M) {
      long const q = mm / nd;
      int const id = (int)(mm - q * nd);
      long const r = n.srays[q0 + q], at = r * nd + id;
      double const yy = n.y[at], wt = n.weight[at];
      double const f = a.out_rad[at];
      // (masked as the forward model masks: any non-finite input; F of a channel that is not masked is finite)
      if (isfinite(a.in_rad[at]) && isfinite(f) && isfinite(yy) && wt > 0) {
        ww = wt;
        d = yy - f;
        if (col < w) v = a.k[(a.rowptr[r] - kbase) * nd + (long)id * w + col];
      }
    }
    rows[buf][lc][lcol] = v;
    if (lcol == 0) { wl[buf][lc] = ww; dl[buf][lc] = d; }
    __syncthreads();
    for (int c = 0; c < 8; c++) {
      double const wc = wl[buf][c];
      if (!(wc > 0)) continue;                            // (uniform)
      double const ki = rows[buf][c][ty], kj = rows[buf][c][16 + tx];
      acc = fma(ki * kj, wc, acc);
      if (with_b || with_cost) {
        double const dc = dl[buf][c], wd = wc * dc;
        if (with_b) acc_b = fma(ki, wd, acc_b);
        if (with_cost) { acc_c = fma(wd, dc, acc_c); count++; }
      }
    }
  }
  if (inside) {
    As[(long)i * w + j] = acc;
    if (tj < ti) As[(long)j * w + i] = acc;
  }
  if (with_b) n.b[n.wptr[s] + i] = acc_b;
  if (with_cost) { n.cost[s] = acc_c; n.nlive[s] = count; }
}

// ---- gradient of a scene from held blocks (jur_gradient_scene_host, reuse iterations of jur_retrieve_scene_host) -----
// A matrix-vector sum over ragged blocks.  One workgroup per 256 consecutive state elements of one slice; lane i owns
// element e = 256 g + i and carries its chain b_e = fma(K[id][e], weight * (y - F), b_e) over the slice's rays of the pass,
// ascending, and their channels, ascending -- jur_scene_normal_kernel's acc_b, operand for operand, from the value the
// earlier passes left.  The measurements are taken GRAD_CH at a time: lane c of the first GRAD_CH stages weight (0: not
// live, by jur_scene_normal_kernel's rule; the measurement is then skipped by all lanes, so that the NaN row of a masked
// channel is never read), y - F and the first double of the block row in one of two LDS buffers (one barrier per group);
// what is staged does not grow with the slice.  The lanes then read entry (id, e) of each live row: consecutive doubles,
// one coalesced stretch per row.  Lane 0 of the slice's first workgroup carries cost and nlive.  No atomics.
#define GRAD_CH 64
__global__ __launch_bounds__(256) void jur_scene_gradient_kernel(jur_scene_pass_t a, jur_scene_normal_t n, jur_scene_grad_t g) {
  __shared__ double wl[2][GRAD_CH], dl[2][GRAD_CH];
  __shared__ long kl[2][GRAD_CH];
  long const s = scene_find<false>(g.gptr, 0, n.nslice, (long)blockIdx.x);
  long const q0 = scene_lower(n.srays, n.sptr[s], n.sptr[s + 1], a.r0), q1 = scene_lower(n.srays, q0, n.sptr[s + 1], a.r1);
  if (q1 == q0) return;                                   // (uniform: before any barrier)
  int const w = (int)(n.wptr[s + 1] - n.wptr[s]), nd = a.nd;
  long const grp = (long)blockIdx.x - g.gptr[s];
  int const lane = threadIdx.x, i = (int)(grp * 256) + lane;
  bool const with_b = i < w, with_cost = grp == 0 && lane == 0;
  double acc_b = with_b ? n.b[n.wptr[s] + i] : 0.;
  double acc_c = with_cost ? n.cost[s] : 0.;
  long count = with_cost ? n.nlive[s] : 0;
  long const M = (q1 - q0) * nd;
  for (long m0 = 0; m0 < M; m0 += GRAD_CH) {
    int const buf = (int)(m0 / GRAD_CH) & 1;
    if (lane < GRAD_CH) {
      long const mm = m0 + lane;
      double ww = 0., d = 0.;
      long at_k = 0;
      if (mm < M) {
        long const q = mm / nd;
        int const id = (int)(mm - q * nd);
        long const r = n.srays[q0 + q], at = r * nd + id;
        double const yy = n.y[at], wt = n.weight[at];
        double const f = a.out_rad[at];
        if (isfinite(a.in_rad[at]) && isfinite(f) && isfinite(yy) && wt > 0) {
          ww = wt;
          d = yy - f;
          at_k = g.koff[r] + (long)id * w;
        }
      }
      wl[buf][lane] = ww; dl[buf][lane] = d; kl[buf][lane] = at_k;
    }
    __syncthreads();
    int const nc = M - m0 < GRAD_CH ? (int)(M - m0) : GRAD_CH;
    for (int c = 0; c < nc; c++) {
      double const wc = wl[buf][c];
      if (!(wc > 0)) continue;                            // (uniform)
      double const dc = dl[buf][c], wd = wc * dc;
      if (with_b) acc_b = fma(g.k[kl[buf][c] + i], wd, acc_b);
      if (with_cost) { acc_c = fma(wd, dc, acc_c); count++; }
    }
  }
  if (with_b) n.b[n.wptr[s] + i] = acc_b;
  if (with_cost) { n.cost[s] = acc_c; n.nlive[s] = count; }
}

// ---- Levenberg-Marquardt step of a scene (jur_solve_slices_host, jur_step_scene_host) -------------------------------
// One workgroup per system: M = L L^T in place in the system's part of the scratch a.M (global memory, L2-resident),
// L z = g and L^T dx = z in a.dx, pred.  Nothing waits on another workgroup, no atomics; every chain of operations is
// fixed by w alone.  A dead element (D_i = A_ii + r_i not > 0) is an identity row and column with g_i = 0: its L_ii is 1,
// it adds exact zeros to the chains of the live elements, and its dx is set to +0.0 at the end.
//
// Right-looking, 16 columns a step: the 16 x 16 diagonal block is factored in LDS (T; a pivot that is not > 0 just before
// its square root ends the system: status 1 + column, L, dx and pred zeroed) and the forward substitution of its 16
// elements of z is done with it; the rows below take one lane each (their 16 entries of the panel in registers, one true
// division per entry, then their z); the trailing update takes the panel from LDS in chunks of 64 rows (PI, PJ: what
// is staged does not grow with w), a 4 x 4 micro-tile of a 64 x 64 piece of the lower triangle per lane.  The back
// substitution walks the blocks upwards, lane i taking column i of the block's rows.  LDS: 21 KB.
#define SOLVE_NB 16
#define SOLVE_CH 64
__global__ __launch_bounds__(256) void jur_scene_solve_kernel(jur_scene_solve_t a) {
  __shared__ double T[SOLVE_NB][SOLVE_NB + 1], zb[SOLVE_NB], dg[SOLVE_NB];
  __shared__ double PI[SOLVE_NB][SOLVE_CH + 1], PJ[SOLVE_NB][SOLVE_CH + 1];
  __shared__ double red[256];
  long const s = blockIdx.x;
  int const tid = threadIdx.x, w = (int)(a.wptr[s + 1] - a.wptr[s]);
  if (w <= 0) {                                             // (uniform)
    if (tid == 0) { a.pred[s] = 0.; a.status[s] = 0; }
    return;
  }
  if (a.state && a.state[s] != 0) return;                   // (uniform) a slice whose retrieval has ended
  double const *const A = a.A + a.aptr[s], *const b = a.b + a.wptr[s];
  double const *const pr = a.prior_ivar ? a.prior_ivar + a.wptr[s] : nullptr;
  double const *const pd = a.prior_ivar ? a.prior_dx + a.wptr[s] : nullptr;
  double *const M = a.M + a.aptr[s], *const lv = a.live + a.wptr[s], *const z = a.dx + a.wptr[s];
  double const lam = a.lam[s];
  bool const by_prior = a.mode == JUR_DAMP_PRIOR;

  // D, liveness, M_ii and g
  for (int i = tid; i < w; i += 256) {
    double const ri = pr ? pr[i] : 0., di = pr ? pd[i] : 0., D = A[(long)i * w + i] + ri;
    bool const live = D > 0;
    lv[i] = live ? D : 0.;
    M[(long)i * w + i] = live ? fma(lam, by_prior ? ri : D, D) : 1.;
    z[i] = live ? fma(ri, di, b[i]) : 0.;
  }
  __syncthreads();
  // the lower triangle between live elements; zeros elsewhere
  for (int i = tid >> 6; i < w; i += 4) {
    bool const li = lv[i] > 0;
    for (int j = tid & 63; j < w; j += 64)
      if (j != i) M[(long)i * w + j] = (j < i && li && lv[j] > 0) ? A[(long)i * w + j] : 0.;
  }
  __syncthreads();

  int const tr = tid >> 4, tc = tid & 15;
  int bad = 0;                                              // 1 + the column of the pivot that is not > 0 (uniform)
  for (int k0 = 0; k0 < w && !bad; k0 += SOLVE_NB) {
    int const nb = min(SOLVE_NB, w - k0);
    if (tr < nb && tc <= tr) T[tr][tc] = M[(long)(k0 + tr) * w + k0 + tc];
    if (tid < nb) zb[tid] = z[k0 + tid];
    __syncthreads();
    for (int k = 0; k < nb; k++) {
      double const piv = T[k][k];                           // (stays as it is: the root goes to dg)
      if (!(piv > 0)) { bad = 1 + k0 + k; break; }          // (every lane reads the same value)
      double const l = sqrt(piv);
      if (tc == k && tr > k && tr < nb) T[tr][k] = T[tr][k] / l;
      if (tid == 0) dg[k] = l;
      __syncthreads();
      if (tr < nb && tc > k && tc <= tr) T[tr][tc] = fma(-T[tr][k], T[tc][k], T[tr][tc]);
      __syncthreads();
    }
    if (bad) break;
    if (tid < nb) T[tid][tid] = dg[tid];
    __syncthreads();
    if (tid == 0)
      for (int c = 0; c < nb; c++) {
        double acc = zb[c];
        for (int k = 0; k < c; k++) acc = fma(-T[c][k], zb[k], acc);
        zb[c] = acc / T[c][c];
      }
    if (tr < nb && tc <= tr) M[(long)(k0 + tr) * w + k0 + tc] = T[tr][tc];
    __syncthreads();
    if (tid < nb) z[k0 + tid] = zb[tid];
    if (k0 + SOLVE_NB >= w) break;                          // (no rows below: nb == SOLVE_NB from here on)
    // the panel: row i of L's 16 columns, then z_i
    for (int i = k0 + SOLVE_NB + tid; i < w; i += 256) {
      double *const row = M + (long)i * w + k0;
      double x[SOLVE_NB];
#pragma unroll
      for (int c = 0; c < SOLVE_NB; c++) x[c] = row[c];
      double zi = z[i];
#pragma unroll
      for (int c = 0; c < SOLVE_NB; c++) {
        double acc = x[c];
#pragma unroll
        for (int k = 0; k < c; k++) acc = fma(-x[k], T[c][k], acc);
        x[c] = acc / T[c][c];
        row[c] = x[c];
        zi = fma(-x[c], zb[c], zi);
      }
      z[i] = zi;
    }
    __syncthreads();
    // the trailing update M_ij -= sum_k L_ik L_jk, k ascending, for k0 + 16 <= j <= i
    for (int I0 = k0 + SOLVE_NB; I0 < w; I0 += SOLVE_CH) {
      for (int e = tid; e < SOLVE_NB * SOLVE_CH; e += 256) {
        int const rr = e >> 4, kk = e & 15, i = I0 + rr;
        PI[kk][rr] = i < w ? M[(long)i * w + k0 + kk] : 0.;
      }
      for (int J0 = k0 + SOLVE_NB; J0 <= I0; J0 += SOLVE_CH) {
        for (int e = tid; e < SOLVE_NB * SOLVE_CH; e += 256) {
          int const rr = e >> 4, kk = e & 15, j = J0 + rr;
          PJ[kk][rr] = j < w ? M[(long)j * w + k0 + kk] : 0.;
        }
        __syncthreads();
        double acc[4][4];
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
          for (int q = 0; q < 4; q++) {
            int const i = I0 + tr + 16 * p, j = J0 + tc + 16 * q;
            acc[p][q] = (i < w && j <= i) ? M[(long)i * w + j] : 0.;
          }
#pragma unroll
        for (int k = 0; k < SOLVE_NB; k++) {
          double pi[4], pj[4];
#pragma unroll
          for (int p = 0; p < 4; p++) { pi[p] = PI[k][tr + 16 * p]; pj[p] = PJ[k][tc + 16 * p]; }
#pragma unroll
          for (int p = 0; p < 4; p++)
#pragma unroll
            for (int q = 0; q < 4; q++) acc[p][q] = fma(-pi[p], pj[q], acc[p][q]);
        }
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
          for (int q = 0; q < 4; q++) {
            int const i = I0 + tr + 16 * p, j = J0 + tc + 16 * q;
            if (i < w && j <= i) M[(long)i * w + j] = acc[p][q];
          }
        __syncthreads();
      }
    }
  }
  if (bad) {
    for (long e = tid; e < (long)w * w; e += 256) M[e] = 0.;
    for (int i = tid; i < w; i += 256) z[i] = 0.;
    if (tid == 0) { a.pred[s] = 0.; a.status[s] = bad; }
    return;
  }
  __syncthreads();

  // L^T dx = z, from the last block upwards
  for (int k0 = ((w - 1) / SOLVE_NB) * SOLVE_NB; k0 >= 0; k0 -= SOLVE_NB) {
    int const nb = min(SOLVE_NB, w - k0);
    if (tr < nb && tc <= tr) T[tr][tc] = M[(long)(k0 + tr) * w + k0 + tc];
    if (tid < nb) zb[tid] = z[k0 + tid];
    __syncthreads();
    if (tid == 0)
      for (int c = nb - 1; c >= 0; c--) {
        double acc = zb[c];
        for (int k = c + 1; k < nb; k++) acc = fma(-T[k][c], zb[k], acc);
        zb[c] = acc / T[c][c];
      }
    __syncthreads();
    if (tid < nb) z[k0 + tid] = zb[tid];
    for (int i = tid; i < k0; i += 256) {
      double zi = z[i];
      for (int k = 0; k < nb; k++) zi = fma(-M[(long)(k0 + k) * w + i], zb[k], zi);
      z[i] = zi;
    }
    __syncthreads();
  }

  // dx of the dead elements, pred: every lane its elements ascending, then a fixed tree over the lanes
  double sum = 0.;
  for (int i = tid; i < w; i += 256) {
    double const D = lv[i];
    if (D > 0) {
      double const ri = pr ? pr[i] : 0., di = pr ? pd[i] : 0., dx = z[i];
      sum += dx * fma(lam * (by_prior ? ri : D), dx, fma(ri, di, b[i]));
    } else z[i] = 0.;
  }
  red[tid] = sum;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) { a.pred[s] = red[0]; a.status[s] = 0; }
}

// ---- posterior diagnostics of a scene (jur_diagnose_slices_host, jur_diagnose_scene_host) ---------------------------
// S = M^-1 from the factor jur_scene_solve_kernel left (lam = 0): L Y = I, then L^T S = Y.  One workgroup per block of 16
// columns (c0 ...) of one system, so a wide system spreads over w / 16 workgroups that share nothing.  Column j of Y is
// zero above row j and rows i >= j of column j of S need only the rows below them, so the workgroup works on the rows
// >= c0 alone, in place in its 16 columns of S: the lower triangle is what is computed, and it is mirrored at the end
// (the rows above c0 of these columns receive the mirror images of the workgroups to the left and are never read here).
// Both substitutions go by blocks of 16 rows: lane (tr, tc) carries element (k0 + tr, c0 + tc) of the block's right-hand
// side as a chain of fused multiply-adds over the rows already solved, ascending, staged through LDS 64 at a time (LT: L,
// YT: the solved rows), then the 16 x 16 diagonal block of L is taken to LDS (T) and lane c < 16 substitutes column c
// of the block (true divisions).  Every chain is fixed by w and the column alone.  A dead element is an identity row and
// column of L; its row and column of S, the diagonal included, are set to +0.0 at the end.  A system that broke down
// (status != 0, L all zeros) gets +0.0 throughout.  LDS: 21 KB.
#define DIAG_NB 16
#define DIAG_KC 64
__global__ __launch_bounds__(256) void jur_scene_inverse_kernel(jur_scene_diag_t a) {
  __shared__ double T[DIAG_NB][DIAG_NB + 1], X[DIAG_NB][DIAG_NB + 1];
  __shared__ double LT[DIAG_KC][DIAG_NB + 1], YT[DIAG_KC][DIAG_NB + 1];
  long const s = a.imap[2 * (long)blockIdx.x];
  int const c0 = a.imap[2 * (long)blockIdx.x + 1];
  int const tid = threadIdx.x, tr = tid >> 4, tc = tid & 15, w = (int)(a.wptr[s + 1] - a.wptr[s]);
  int const nc = min(DIAG_NB, w - c0);
  double const *const L = a.L + a.aptr[s], *const lv = a.live + a.wptr[s];
  double *const S = a.S + a.aptr[s];
  if (a.status[s] != 0) {                                   // (uniform)
    for (long e = tid; e < (long)w * DIAG_NB; e += 256) {
      int const i = (int)(e >> 4), c = (int)(e & 15);
      if (c < nc) S[(long)i * w + c0 + c] = 0.;
    }
    return;
  }

  // L Y = I, from the block of the diagonal downwards
  for (int k0 = c0; k0 < w; k0 += DIAG_NB) {
    int const nb = min(DIAG_NB, w - k0);
    double acc = (k0 == c0 && tr == tc) ? 1. : 0.;
    for (int kk = c0; kk < k0; kk += DIAG_KC) {
      int const kn = min(DIAG_KC, k0 - kk);                 // (a multiple of 16)
      for (int e = tid; e < DIAG_NB * DIAG_KC; e += 256) {
        int const r = e >> 6, k = e & 63;
        LT[k][r] = (r < nb && k < kn) ? L[(long)(k0 + r) * w + kk + k] : 0.;
      }
      for (int e = tid; e < DIAG_NB * DIAG_KC; e += 256) {
        int const k = e >> 4, c = e & 15;
        YT[k][c] = (k < kn && c < nc) ? S[(long)(kk + k) * w + c0 + c] : 0.;
      }
      __syncthreads();
#pragma unroll 16
      for (int k = 0; k < kn; k++) acc = fma(-LT[k][tr], YT[k][tc], acc);
      __syncthreads();
    }
    if (tr < nb && tc <= tr) T[tr][tc] = L[(long)(k0 + tr) * w + k0 + tc];
    X[tr][tc] = acc;
    __syncthreads();
    if (tid < nc)
      for (int r = 0; r < nb; r++) {
        double v = X[r][tid];
        for (int k = 0; k < r; k++) v = fma(-T[r][k], X[k][tid], v);
        X[r][tid] = v / T[r][r];
      }
    __syncthreads();
    if (tr < nb && tc < nc) S[(long)(k0 + tr) * w + c0 + tc] = X[tr][tc];
    __syncthreads();
  }

  // L^T S = Y, from the last block upwards to the block of the diagonal
  for (int k0 = ((w - 1) / DIAG_NB) * DIAG_NB; k0 >= c0; k0 -= DIAG_NB) {
    int const nb = min(DIAG_NB, w - k0);
    double acc = (tr < nb && tc < nc) ? S[(long)(k0 + tr) * w + c0 + tc] : 0.;
    for (int kk = k0 + DIAG_NB; kk < w; kk += DIAG_KC) {
      int const kn = min(DIAG_KC, w - kk);
      for (int e = tid; e < DIAG_NB * DIAG_KC; e += 256) {
        int const k = e >> 4, c = e & 15;
        bool const in = k < kn;
        LT[k][c] = in ? L[(long)(kk + k) * w + k0 + c] : 0.;   // (rows below exist: the block k0 is a full one)
        YT[k][c] = (in && c < nc) ? S[(long)(kk + k) * w + c0 + c] : 0.;
      }
      __syncthreads();
      for (int k = 0; k < kn; k++) acc = fma(-LT[k][tr], YT[k][tc], acc);
      __syncthreads();
    }
    if (tr < nb && tc <= tr) T[tr][tc] = L[(long)(k0 + tr) * w + k0 + tc];
    X[tr][tc] = acc;
    __syncthreads();
    if (tid < nc)
      for (int r = nb - 1; r >= 0; r--) {
        double v = X[r][tid];
        for (int k = r + 1; k < nb; k++) v = fma(-T[k][r], X[k][tid], v);
        X[r][tid] = v / T[r][r];
      }
    __syncthreads();
    if (tr < nb && tc < nc) S[(long)(k0 + tr) * w + c0 + tc] = X[tr][tc];
    __syncthreads();
  }

  // the dead elements, and the mirror image of what lies below the diagonal
  for (long e = tid; e < (long)(w - c0) * DIAG_NB; e += 256) {
    int const i = c0 + (int)(e >> 4), j = c0 + (int)(e & 15);
    if (j >= w || i < j) continue;
    double v = S[(long)i * w + j];
    if (!(lv[i] > 0) || !(lv[j] > 0)) { v = 0.; S[(long)i * w + j] = v; }
    if (i > j) S[(long)j * w + i] = v;
  }
}

// AVK = S A.  One workgroup per 64 x 64 tile of one system's AVK; lane (tr, tc) holds the 4 x 4 micro-tile of the
// elements (i0 + tr + 16 p, j0 + tc + 16 q) and carries each as one chain of fused multiply-adds over k = 0 .. w - 1,
// ascending (padded with exact zeros to a multiple of 16), the operands staged through LDS 16 values of k at a time: SI
// the tile's rows of S, AJ its columns of A.  Of A only the diagonal and the lower triangle are read (A_kj from
// A[max][min]), and an entry in the row or column of a dead element counts as 0, whatever the caller left there.  The
// rows and columns of dead elements, and a system that broke down, are written as +0.0.  LDS: 17 KB.
#define DIAG_TILE 64
__global__ __launch_bounds__(256) void jur_scene_avk_kernel(jur_scene_diag_t a) {
  __shared__ double SI[DIAG_NB][DIAG_TILE + 1], AJ[DIAG_NB][DIAG_TILE + 1];
  long const s = a.tmap[3 * (long)blockIdx.x];
  int const i0 = a.tmap[3 * (long)blockIdx.x + 1], j0 = a.tmap[3 * (long)blockIdx.x + 2];
  int const tid = threadIdx.x, tr = tid >> 4, tc = tid & 15, w = (int)(a.wptr[s + 1] - a.wptr[s]);
  double const *const A = a.A + a.aptr[s], *const S = a.S + a.aptr[s], *const lv = a.live + a.wptr[s];
  double *const K = a.avk + a.aptr[s];
  bool const bad = a.status[s] != 0;                        // (uniform)
  double acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; p++)
#pragma unroll
    for (int q = 0; q < 4; q++) acc[p][q] = 0.;
  for (int k0 = 0; k0 < w && !bad; k0 += DIAG_NB) {
    for (int e = tid; e < DIAG_NB * DIAG_TILE; e += 256) {
      int const rr = e >> 4, kk = e & 15, i = i0 + rr, k = k0 + kk;
      SI[kk][rr] = (i < w && k < w) ? S[(long)i * w + k] : 0.;
    }
    for (int e = tid; e < DIAG_NB * DIAG_TILE; e += 256) {
      int const kk = e >> 6, cc = e & 63, k = k0 + kk, j = j0 + cc;
      double v = 0.;
      if (k < w && j < w && lv[k] > 0 && lv[j] > 0) v = k >= j ? A[(long)k * w + j] : A[(long)j * w + k];
      AJ[kk][cc] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < DIAG_NB; k++) {
      double si[4], aj[4];
#pragma unroll
      for (int p = 0; p < 4; p++) { si[p] = SI[k][tr + 16 * p]; aj[p] = AJ[k][tc + 16 * p]; }
#pragma unroll
      for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[p][q] = fma(si[p], aj[q], acc[p][q]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int p = 0; p < 4; p++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      int const i = i0 + tr + 16 * p, j = j0 + tc + 16 * q;
      if (i < w && j < w) K[(long)i * w + j] = (bad || !(lv[i] > 0) || !(lv[j] > 0)) ? 0. : acc[p][q];
    }
}

// The vectors, one wavefront per element e = (system s, row i): avk_diag = AVK_ii, sigma = sqrt(S_ii), and the two sums
// over the row, sum_j AVK_ij S_ij (S_ji has the same bits) and sum_j S_ij^2 r_j: lane l takes j = l, l + 64, ... ascending
// as a chain of fused multiply-adds, then a fixed tree runs over the 64 lanes.  No LDS, no barrier.
__global__ __launch_bounds__(256) void jur_scene_diag_rows_kernel(jur_scene_diag_t a) {
  long const nb = a.wptr[a.nslice], e = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= nb) return;                                      // (uniform in the wavefront)
  int const lane = threadIdx.x & 63;
  long const s = scene_find<false>(a.wptr, 0, a.nslice, e);
  int const w = (int)(a.wptr[s + 1] - a.wptr[s]), i = (int)(e - a.wptr[s]);
  double const *const Si = a.S + a.aptr[s] + (long)i * w, *const Ki = a.avk + a.aptr[s] + (long)i * w;
  double const *const r = a.prior_ivar ? a.prior_ivar + a.wptr[s] : nullptr;
  double noise = 0., smooth = 0.;
  for (int j = lane; j < w; j += 64) {
    double const sij = Si[j];
    noise = fma(Ki[j], sij, noise);
    if (r) smooth = fma(sij * sij, r[j], smooth);
  }
  for (int h = 32; h > 0; h >>= 1) {
    noise += __shfl_down(noise, h, 64);
    smooth += __shfl_down(smooth, h, 64);
  }
  if (lane == 0) {
    a.avk_diag[e] = Ki[i];
    a.sigma[e] = sqrt(Si[i]);
    a.sigma_noise[e] = sqrt(noise > 0 ? noise : 0.);
    a.sigma_smooth[e] = sqrt(smooth);
  }
}

// dofs[s] = sum_i AVK_ii, one workgroup per system: every lane its elements ascending, then a fixed tree over the lanes
__global__ __launch_bounds__(256) void jur_scene_dofs_kernel(jur_scene_diag_t a) {
  __shared__ double red[256];
  long const s = blockIdx.x;
  int const tid = threadIdx.x, w = (int)(a.wptr[s + 1] - a.wptr[s]);
  double const *const d = a.avk_diag + a.wptr[s];
  double sum = 0.;
  for (int i = tid; i < w; i += 256) sum += d[i];
  red[tid] = sum;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) a.dofs[s] = red[0];
}

// ---- gain matrix and error budget of a scene (jur_gain_slices_host, jur_gain_scene_host) ----------------------------
// The effective weights of a scene: the weight where the measurement is live by jur_scene_normal_kernel's rule (mask: the
// caller's radiances, with a field of view the effective mask), 0 otherwise.  One lane per measurement.
__global__ __launch_bounds__(256) void jur_scene_weff_kernel(jur_scene_weff_t a) {
  long const g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= a.n) return;
  double const wt = a.weight[g];
  a.weff[g] = (isfinite(a.mask[g]) && isfinite(a.f[g]) && isfinite(a.y[g]) && wt > 0) ? wt : 0.;
}

// G = S K^T W, a ragged batched product.  One workgroup per tile of 64 measurements x 64 state elements of one slice
// (gmap: slice, first measurement, first element).  Measurement m of the slice is channel m % nd of its ray m / nd, the
// rays ascending (srays, sptr); its block row starts at k + koff[ray] + channel * w, and its gain row at the same place in
// `gain`.  Lane (tr, tc) holds the 4 x 4 micro-tile of the measurements m0 + tr + 16 p and the elements i0 + tc + 16 q and
// carries each as one chain c = fma(S_ij, K_m[j], c) over j = 0 .. w - 1, ascending (padded with exact zeros to a multiple
// of 16), the operands staged through LDS 16 values of j at a time: SI the tile's rows of S, KM the tile's block rows.  A
// dead j (S_jj not > 0) is staged as zeros on both sides and a measurement that is not live (omega not > 0) as a row of
// zeros: their block entries are never read.  Rows of measurements that are not live, columns of dead elements and a
// system that broke down are written as +0.0; everything else as omega * c.  LDS: 18 KB, two barriers per 16 values of j.
#define GAIN_TILE 64
#define GAIN_NB 16
__global__ __launch_bounds__(256) void jur_scene_gain_kernel(jur_scene_gain_t a) {
  __shared__ double SI[GAIN_NB][GAIN_TILE + 1], KM[GAIN_NB][GAIN_TILE + 1];
  __shared__ double om[GAIN_TILE], dj[GAIN_NB];
  __shared__ long row[GAIN_TILE];
  long const s = a.gmap[3 * (long)blockIdx.x];
  int const m0 = a.gmap[3 * (long)blockIdx.x + 1], i0 = a.gmap[3 * (long)blockIdx.x + 2];
  int const tid = threadIdx.x, tr = tid >> 4, tc = tid & 15, w = (int)(a.wptr[s + 1] - a.wptr[s]), nd = a.nd;
  double const *const S = a.S + a.aptr[s];
  long const q0 = a.sptr[s], M = (a.sptr[s + 1] - q0) * nd;
  bool const bad = a.status && a.status[s] != 0;            // (uniform)
  if (tid < GAIN_TILE) {
    long const mm = (long)m0 + tid;
    long at = -1;
    double ww = 0.;
    if (mm < M) {
      long const q = mm / nd;
      int const id = (int)(mm - q * nd);
      long const r = a.srays[q0 + q];
      double const wt = a.weff[r * nd + id];
      at = a.koff[r] + (long)id * w;
      if (wt > 0) ww = wt;
    }
    row[tid] = at; om[tid] = ww;
  }
  double acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; p++)
#pragma unroll
    for (int q = 0; q < 4; q++) acc[p][q] = 0.;
  for (int j0 = 0; j0 < w && !bad; j0 += GAIN_NB) {
    if (tid < GAIN_NB) { int const j = j0 + tid; dj[tid] = j < w ? S[(long)j * w + j] : 0.; }
    __syncthreads();                                        // (also: the micro-tiles of the last 16 have been taken)
    for (int e = tid; e < GAIN_NB * GAIN_TILE; e += 256) {
      int const rr = e >> 4, jj = e & 15, i = i0 + rr, j = j0 + jj;
      SI[jj][rr] = (i < w && dj[jj] > 0) ? S[(long)i * w + j] : 0.;
      KM[jj][rr] = (om[rr] > 0 && dj[jj] > 0) ? a.k[row[rr] + j] : 0.;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < GAIN_NB; j++) {
      double km[4], si[4];
#pragma unroll
      for (int p = 0; p < 4; p++) { km[p] = KM[j][tr + 16 * p]; si[p] = SI[j][tc + 16 * p]; }
#pragma unroll
      for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[p][q] = fma(si[q], km[p], acc[p][q]);
    }
  }
  if (bad || w <= 0) __syncthreads();                       // (row and om are read below; the loop's barriers did not run)
#pragma unroll
  for (int p = 0; p < 4; p++) {
    int const ml = tr + 16 * p;
    long const at = row[ml];
    if (at < 0) continue;
    double const ww = om[ml];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      int const i = i0 + tc + 16 * q;
      if (i < w) a.gain[at + i] = (bad || !(ww > 0) || !(S[(long)i * w + i] > 0)) ? 0. : ww * acc[p][q];
    }
  }
}

// The error budget: sigma_comp[c][e] = sqrt(sum over the live measurements m of the slice, ascending, of G_em^2 var_c[m]).
// One workgroup per 256 consecutive state elements of one slice (gptr, as jur_scene_gradient_kernel); lane i owns element
// 256 g + i and up to 8 chains q_c = fma(g * g, var_c, q_c), g * g rounded first.  The measurements are taken GRAD_CH at a
// time: the first double of the gain row (-1: not live, the measurement is skipped by all lanes and its variances are
// never read) and the ncomp variances are staged in one of two LDS buffers, one barrier per group; what is staged does
// not grow with the slice.  The lanes then read entry e of each live gain row: one coalesced stretch per row.
__global__ __launch_bounds__(256) void jur_scene_budget_kernel(jur_scene_gain_t a) {
  __shared__ double vl[2][8][GRAD_CH];
  __shared__ long kl[2][GRAD_CH];
  long const s = scene_find<false>(a.gptr, 0, a.nslice, (long)blockIdx.x);
  int const w = (int)(a.wptr[s + 1] - a.wptr[s]), nd = a.nd, ncomp = a.ncomp;
  long const grp = (long)blockIdx.x - a.gptr[s];
  int const lane = threadIdx.x, i = (int)(grp * 256) + lane;
  bool const inside = i < w;
  long const q0 = a.sptr[s], M = (a.sptr[s + 1] - q0) * nd;
  double q[8];
#pragma unroll
  for (int c = 0; c < 8; c++) q[c] = 0.;
  for (long m0 = 0; m0 < M; m0 += GRAD_CH) {
    int const buf = (int)(m0 / GRAD_CH) & 1;
    for (int e = lane; e < GRAD_CH * ncomp; e += 256) {
      int const c = e / GRAD_CH, ml = e % GRAD_CH;
      long const mm = m0 + ml;
      long at_k = -1;
      double v = 0.;
      if (mm < M) {
        long const qq = mm / nd;
        int const id = (int)(mm - qq * nd);
        long const r = a.srays[q0 + qq], at = r * nd + id;
        if (a.weff[at] > 0) {
          at_k = a.koff[r] + (long)id * w;
          v = a.var[(long)c * a.nrd + at];
        }
      }
      vl[buf][c][ml] = v;
      if (c == 0) kl[buf][ml] = at_k;
    }
    __syncthreads();
    int const nc = M - m0 < GRAD_CH ? (int)(M - m0) : GRAD_CH;
    for (int m = 0; m < nc; m++) {
      long const at = kl[buf][m];
      if (at < 0) continue;                                 // (uniform)
      double const g = inside ? a.gain[at + i] : 0., gg = g * g;
#pragma unroll
      for (int c = 0; c < 8; c++)
        if (c < ncomp) q[c] = fma(gg, vl[buf][c][m], q[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < 8; c++)
    if (c < ncomp && inside) a.sigc[(long)c * a.nb + a.wptr[s] + i] = sqrt(q[c]);
}

// ---- parameter errors of a scene (jur_param_slices_host) --------------------------------------------------------------
// C_s = G_s^T Kb_s, a ragged batched contraction over the measurements.  One workgroup per tile of 64 state elements x 64
// parameters of one slice (cmap: slice, first element, first parameter).  Measurement m of the slice is channel m % nd of
// its ray m / nd, the rays ascending (srays, sptr); its gain row starts at gain + koff[ray] + channel * w and its kb row
// at kb + koffb[ray] + channel * wb.  Lane (tr, tc) holds the 4 x 4 micro-tile of the elements i0 + tr + 16 p and the
// parameters j0 + tc + 16 q and carries each as one chain c = fma(G_m,i, Kb_m,j, c) over all measurements of the slice,
// ascending, the operands staged through LDS 16 measurements at a time: GI the tile's 64 gain entries of each, KB its 64
// kb entries.  Wavefront v stages the measurements v, v + 4, v + 8, v + 12 of the 16, a lane per entry: the row address
// and the liveness are uniform in the wavefront and the 64 entries one contiguous stretch.  A measurement that is not
// live (omega not > 0), and what lies beyond the slice's measurements or beyond w or wb, is staged as exact zeros and
// never loaded; fma(+0, +0, c) leaves every chain as it was.  The lanes of a wavefront read two neighbouring doubles of a
// GI row (broadcast to 16 lanes each) and 16 consecutive doubles of a KB row: no bank conflicts, so the rows need none
// of the padding jur_scene_gain_kernel's transposed staging needs.  LDS: 16 KB, two barriers per 16 measurements.
//
// PASS (jur_param_scene_host): the same chains over the rays of one pass.  The tile comes with the stretch [lo, hi) of
// srays that holds the rays of its slice inside the pass (pmap: slice, first element, first parameter, lo, hi); every
// chain starts from the value C holds -- +0.0 before the first pass -- and is stored back, and the kb row of a ray lies
// in the buffer of the pass, kb0 doubles before where koffb puts it.  The measurements of a slice are taken in the same
// ascending order, 16 at a time from lo: only the exact zeros that pad a stretch to 16 move with the cuts.
#define CROSS_TILE 64
#define CROSS_NB 16
template <bool PASS>
__device__ __forceinline__ void scene_cross_body(jur_scene_param_t const &a, int const *map, long kb0) {
  __shared__ double GI[CROSS_NB][CROSS_TILE], KB[CROSS_NB][CROSS_TILE];
  int const *const tile = map + (PASS ? 5 : 3) * (long)blockIdx.x;
  long const s = tile[0];
  int const i0 = tile[1], j0 = tile[2];
  int const tid = threadIdx.x, tr = tid >> 4, tc = tid & 15, col = tid & 63, wv = tid >> 6, nd = a.nd;
  int const w = (int)(a.wptr[s + 1] - a.wptr[s]), wb = (int)(a.bwptr[s + 1] - a.bwptr[s]);
  long const q0 = PASS ? (long)tile[3] : a.sptr[s], M = ((PASS ? (long)tile[4] : a.sptr[s + 1]) - q0) * nd;
  bool const gi_in = i0 + col < w, kb_in = j0 + col < wb;
  double *const C = a.C + a.cptr[s];
  double acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; p++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      int const i = i0 + tr + 16 * p, j = j0 + tc + 16 * q;
      acc[p][q] = (PASS && i < w && j < wb) ? C[(long)i * wb + j] : 0.;
    }
  for (long m0 = 0; m0 < M; m0 += CROSS_NB) {
    __syncthreads();                                        // (the micro-tiles of the last 16 have been taken)
#pragma unroll
    for (int t = 0; t < CROSS_NB / 4; t++) {
      int const ml = wv + 4 * t;
      long const mm = m0 + ml;
      double g = 0., kb = 0.;
      if (mm < M) {                                         // (uniform in the wavefront, as is the liveness)
        long const qq = mm / nd;
        int const id = (int)(mm - qq * nd);
        long const r = a.srays[q0 + qq];
        if (a.weff[r * nd + id] > 0) {
          if (gi_in) g = a.gain[a.koff[r] + (long)id * w + i0 + col];
          if (kb_in) kb = a.kb[a.koffb[r] - kb0 + (long)id * wb + j0 + col];
        }
      }
      GI[ml][col] = g; KB[ml][col] = kb;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < CROSS_NB; m++) {
      double gi[4], kj[4];
#pragma unroll
      for (int p = 0; p < 4; p++) { gi[p] = GI[m][tr + 16 * p]; kj[p] = KB[m][tc + 16 * p]; }
#pragma unroll
      for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[p][q] = fma(gi[p], kj[q], acc[p][q]);
    }
  }
#pragma unroll
  for (int p = 0; p < 4; p++) {
    int const i = i0 + tr + 16 * p;
    if (i >= w) continue;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      int const j = j0 + tc + 16 * q;
      if (j < wb) C[(long)i * wb + j] = acc[p][q];
    }
  }
}
__global__ __launch_bounds__(256) void jur_scene_cross_kernel(jur_scene_param_t a) { scene_cross_body<false>(a, a.cmap, 0); }
__global__ __launch_bounds__(256) void jur_scene_cross_pass_kernel(jur_scene_param_t a, int const *pmap, long kb0) {
  scene_cross_body<true>(a, pmap, kb0);
}

// The quadratic forms on C_s: sigma_param[c][e] = sqrt(diag(C Sigma_c C^T)) for up to 8 components, the diagonal ones
// first.  One workgroup of four wavefronts per 64 consecutive state elements (rows of C_s) of one slice (pptr); lane l of
// every wavefront has row 64 g + l.  What is staged is 64 rows x 16 columns of C (CL, and CJ for the outer index of a
// full component), 16 x 16 of Sigma (SG), the 16 variances of every diagonal component (VL) and 64 x 16 partial
// vectors (TT), whatever the slice.  Rows are padded to 17 doubles: the lanes of a wavefront read one column of 64 rows.
// Diagonal component c: wavefront c % 4 carries q = fma(C_ij * C_ij, var_j, q) over j ascending, the square rounded first.
// Full component c: for every 16 values of j the four wavefronts carry four each of the chains t_j = fma(Sigma_jl, C_il, t)
// over l ascending (Sigma_jl for l > j read as Sigma_lj; its entry is uniform in the wavefront: a broadcast), leave them
// in TT, and wavefront c % 4 extends q = fma(C_ij, t_j, q) over these j, ascending.  Columns beyond wb are staged as
// exact zeros and never loaded.  sqrt(q) where q > 0 or q is NaN, +0.0 otherwise.
#define PARAM_ROWS 64
#define PARAM_NB 16
__device__ inline void param_stage_rows(double (*T)[PARAM_NB + 1], double const *C, int i0, int c0, int w, int wb, int tid) {
  for (int e = tid; e < PARAM_ROWS * PARAM_NB; e += 256) {
    int const rr = e >> 4, cc = e & 15, i = i0 + rr, j = c0 + cc;
    T[rr][cc] = (i < w && j < wb) ? C[(long)i * wb + j] : 0.;
  }
}
__global__ __launch_bounds__(256) void jur_scene_param_kernel(jur_scene_param_t a) {
  __shared__ double CL[PARAM_ROWS][PARAM_NB + 1], CJ[PARAM_ROWS][PARAM_NB + 1], TT[PARAM_ROWS][PARAM_NB + 1];
  __shared__ double SG[PARAM_NB][PARAM_NB + 1], VL[8][PARAM_NB];
  long const s = scene_find<false>(a.pptr, 0, a.nslice, (long)blockIdx.x);
  int const w = (int)(a.wptr[s + 1] - a.wptr[s]), wb = (int)(a.bwptr[s + 1] - a.bwptr[s]);
  int const tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nvar = a.nvar, ncov = a.ncov;
  int const i0 = (int)(((long)blockIdx.x - a.pptr[s]) * PARAM_ROWS), i = i0 + lane;
  bool const inside = i < w;
  double const *const C = a.C + a.cptr[s];
  double *const out = a.sig + a.wptr[s] + i;
  if (nvar > 0) {
    double qa = 0., qb = 0.;                                // (the components wv and wv + 4)
    for (int j0 = 0; j0 < wb; j0 += PARAM_NB) {
      __syncthreads();                                      // (the last 16 columns have been taken)
      param_stage_rows(CL, C, i0, j0, w, wb, tid);
      if (tid < nvar * PARAM_NB) {
        int const c = tid >> 4, j = j0 + (tid & 15);
        VL[c][tid & 15] = j < wb ? a.var[(long)c * a.nbw + a.bwptr[s] + j] : 0.;
      }
      __syncthreads();
#pragma unroll
      for (int jj = 0; jj < PARAM_NB; jj++) {
        double const cij = CL[lane][jj], cc = cij * cij;
        if (wv < nvar) qa = fma(cc, VL[wv][jj], qa);
        if (wv + 4 < nvar) qb = fma(cc, VL[wv + 4][jj], qb);
      }
    }
    if (inside && wv < nvar) out[(long)wv * a.nb] = (qa > 0 || qa != qa) ? sqrt(qa) : 0.;
    if (inside && wv + 4 < nvar) out[(long)(wv + 4) * a.nb] = (qb > 0 || qb != qb) ? sqrt(qb) : 0.;
  }
  for (int c = 0; c < ncov; c++) {
    double const *const Sg = a.cov + (long)c * a.nbb + a.bbptr[s];
    bool const mine = wv == ((nvar + c) & 3);               // (the wavefront that carries q of this component)
    double q = 0.;
    for (int j0 = 0; j0 < wb; j0 += PARAM_NB) {
      double t[4] = {0., 0., 0., 0.};                       // (t_j of j = j0 + 4 wv + u)
      for (int l0 = 0; l0 < wb; l0 += PARAM_NB) {
        __syncthreads();                                    // (the last tiles, and TT and CJ of the last j0, have been taken)
        param_stage_rows(CL, C, i0, l0, w, wb, tid);
        if (l0 == 0) param_stage_rows(CJ, C, i0, j0, w, wb, tid);
        {
          int const jj = tid >> 4, ll = tid & 15, j = j0 + jj, l = l0 + ll;
          SG[jj][ll] = (j < wb && l < wb) ? (l <= j ? Sg[(long)j * wb + l] : Sg[(long)l * wb + j]) : 0.;
        }
        __syncthreads();
#pragma unroll
        for (int ll = 0; ll < PARAM_NB; ll++) {
          double const cil = CL[lane][ll];
#pragma unroll
          for (int u = 0; u < 4; u++) t[u] = fma(SG[4 * wv + u][ll], cil, t[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; u++) TT[lane][4 * wv + u] = t[u];
      __syncthreads();
      if (mine) {
#pragma unroll
        for (int jj = 0; jj < PARAM_NB; jj++) q = fma(CJ[lane][jj], TT[lane][jj], q);
      }
    }
    if (mine && inside) out[(long)(nvar + c) * a.nb] = (q > 0 || q != q) ? sqrt(q) : 0.;
  }
}

// ---- trial states of a scene (jur_trial_scene_host, jur_retrieve_scene_host) -----------------------------------------
// One lane per state element e of slice s (JUR_ELEM_APPLY: per trial t and element).  The value of element e is
// base[erow[e]][eip[e]]; its place in trial copy 1 + s * ntrial + t is the same row at off[copy] + (eip[e] - sfirst[s]).
//   JUR_ELEM_APPLY     rows[copy of (s, t)] = x_e + dx[t][e], one IEEE addition (after jur_scene_stack_kernel has copied
//                      the slices as they stand: stream order, no lane writes what another reads)
//   JUR_ELEM_PRIOR_DX  out[e] = xa[e] - x_e
//   JUR_ELEM_ACCEPT    x_e += dx[choice[s]][e] in the base rows where choice[s] >= 0
//   JUR_ELEM_STATE     out[e] = x_e
// With a box on the state (a.lo, a.hi: jur_model_set_state_bounds) the sum of JUR_ELEM_APPLY and JUR_ELEM_ACCEPT is bounded
// by JUR_STATE_BOUND, the host's text, before it is stored: the branch is uniform over the launch.
__global__ __launch_bounds__(256) void jur_scene_elements_kernel(jur_scene_trial_t a, int op) {
  long const g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long const nb = a.wptr[a.nslice];
  if (g >= (op == JUR_ELEM_APPLY ? nb * a.ntrial : nb)) return;
  long const t = g / nb, e = g - t * nb;
  long const s = scene_find<false>(a.wptr, 0, a.nslice, e);
  if (a.state && a.state[s] != 0 && op != JUR_ELEM_STATE) return;
  long const at = (long)a.erow[e] * a.np0 + a.eip[e];
  double const x = a.base[at];
  if (op == JUR_ELEM_APPLY) {
    long const copy = 1 + s * a.ntrial + t;
    double v = x + a.dx[g];
    if (a.lo) JUR_STATE_BOUND(v, v, a.lo[e], a.hi[e]);
    a.rows[(long)a.erow[e] * a.nt + a.off[copy] + (a.eip[e] - a.sfirst[s])] = v;
  } else if (op == JUR_ELEM_PRIOR_DX) a.out[e] = a.xa[e] - x;
  else if (op == JUR_ELEM_ACCEPT) {
    int const c = a.choice[s];
    if (c >= 0) {
      double v = x + a.dx[(long)c * nb + e];
      if (a.lo) JUR_STATE_BOUND(v, v, a.lo[e], a.hi[e]);
      a.base[at] = v;
    }
  } else a.out[e] = x;
}

// One lane per (trial, slice): the prior term as the fixed chain d = xa - (x + dx); t = r * d; t = t * d; acc = acc + t
// over the slice's elements ascending (this file is compiled without contraction: four roundings per element).  With a box
// on the state the sum x + dx is bounded first, as JUR_ELEM_APPLY bounds it; the state as it stands (dx == NULL) never is.
__global__ __launch_bounds__(64) void jur_scene_prior_kernel(jur_scene_trial_t a) {
  long const g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int const nrow = a.dx ? a.ntrial : 1;
  if (g >= a.nslice * nrow) return;
  long const t = g / a.nslice, s = g - t * a.nslice;
  if (a.state && a.state[s] != 0) return;
  long const nb = a.wptr[a.nslice];
  double acc = 0.;
  for (long e = a.wptr[s]; e < a.wptr[s + 1]; e++) {
    double x = a.base[(long)a.erow[e] * a.np0 + a.eip[e]];
    if (a.dx) {
      x = x + a.dx[t * nb + e];
      if (a.lo) JUR_STATE_BOUND(x, x, a.lo[e], a.hi[e]);   // (the trial state as JUR_ELEM_APPLY stores it)
    }
    double const d = a.xa[e] - x;
    double term = a.ivar[e] * d;
    term = term * d;
    acc = acc + term;
  }
  a.prior[g] = acc;
}

// Replicated geometry and mask of a pass of trial rays, one lane per slot: trial t of ray r carries the time stamp of
// copy tcopy0[r] + t; a ray without state elements is traced through the base block as jur_scene_rays_kernel's copy 0.
__global__ __launch_bounds__(256) void jur_scene_trial_rays_kernel(jur_scene_trial_pass_t a) {
  long const s = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= a.n) return;
  long const r = a.r0 + s / a.ntrial, t = s - (r - a.r0) * a.ntrial;
  double time;
  if (a.tcopy0[r] > 0) time = a.atm_time[a.off[a.tcopy0[r] + t]];
  else time = a.len[r] >= 2 ? a.atm_time[a.first[r]] : a.above;
  a.geom[s] = time;
  for (int q = 1; q < 7; q++) a.geom[q * a.n + s] = a.in_geom[q * a.nr + r];
  for (int id = 0; id < a.nd; id++) a.rad[s * a.nd + id] = a.in_rad[r * a.nd + id];
}

// One wavefront per (slice, trial): cost[t][s] continues jur_scene_normal_kernel's chain acc = fma(weight * d, d, acc),
// d = y - F, over the slice's rays of the pass, ascending, and their channels, ascending, from the value the earlier
// passes left.  64 measurements at a time are fetched by the lanes and chained by lane 0.  Live: the rule of
// jur_scene_normal_kernel on the inputs; a trial radiance that is not finite makes d, and with it this cost, NaN.
__global__ __launch_bounds__(64) void jur_scene_trial_cost_kernel(jur_scene_trial_pass_t a) {
  __shared__ double wl[64], dl[64];
  long const s = (long)blockIdx.x / a.ntrial, t = (long)blockIdx.x - s * a.ntrial;
  if (a.state && a.state[s] != 0) return;                  // (uniform)
  long const q0 = scene_lower(a.srays, a.sptr[s], a.sptr[s + 1], a.r0), q1 = scene_lower(a.srays, q0, a.sptr[s + 1], a.r1);
  if (q1 == q0) return;                                     // (uniform: before any barrier)
  int const lane = threadIdx.x, nd = a.nd;
  double acc = a.cost[t * a.nslice + s];
  long const M = (q1 - q0) * nd;
  for (long m0 = 0; m0 < M; m0 += 64) {
    long const mm = m0 + lane;
    double ww = 0., d = 0.;
    if (mm < M) {
      long const q = mm / nd;
      int const id = (int)(mm - q * nd);
      long const r = a.srays[q0 + q], at = r * nd + id;
      double const yy = a.y[at], wt = a.weight[at];
      if (isfinite(a.in_rad[at]) && isfinite(yy) && wt > 0) {
        double const f = a.rad[((r - a.r0) * a.ntrial + t) * nd + id];
        ww = wt;
        d = isfinite(f) ? yy - f : __builtin_nan("");
      }
    }
    wl[lane] = ww; dl[lane] = d;
    __syncthreads();
    if (lane == 0)
      for (int c = 0; c < 64; c++) {
        double const wc = wl[c];
        if (!(wc > 0)) continue;
        double const dc = dl[c], wd = wc * dc;
        acc = fma(wd, dc, acc);
      }
    __syncthreads();
  }
  if (lane == 0) a.cost[t * a.nslice + s] = acc;
}

// the rays act[i] of a call in arrays of their own, one lane per gathered ray
__global__ __launch_bounds__(256) void jur_scene_compact_kernel(jur_scene_compact_t a) {
  long const i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  long const r = a.act[i];
  for (int q = 0; q < 7; q++) a.geom_c[q * a.n + i] = a.geom[q * a.nr + r];
  for (int id = 0; id < a.nd; id++) {
    a.rad_c[i * a.nd + id] = a.rad[r * a.nd + id];
    a.y_c[i * a.nd + id] = a.y[r * a.nd + id];
    a.weight_c[i * a.nd + id] = a.weight[r * a.nd + id];
    if (a.live) a.live_c[i * a.nd + id] = a.live[r * a.nd + id];
  }
  a.first_c[i] = a.first[r]; a.len_c[i] = a.len[r]; a.copy0_c[i] = a.copy0[r]; a.tcopy0_c[i] = a.tcopy0[r];
}

// Untraceable rays of a pass (jur_model_set_scene_overflow), one lane per slot, after the pass's forward model and before
// the next pass overwrites np: where JUR_NP_OVERFLOWS(np[slot]) the flag of the slot's (trial, slice) is set.  No atomics:
// every store is the same constant, so the lanes of one cell may store in any order.  The rule reads the ray's own count
// alone -- not the status word, which all slices share.
__global__ __launch_bounds__(256) void jur_scene_overflow_kernel(jur_scene_ovf_t a) {
  long const i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  if (!JUR_NP_OVERFLOWS(a.np[i])) return;
  long r, t = 0;
  if (a.ntrial > 0) { r = a.r0 + i / a.ntrial; t = i - (r - a.r0) * a.ntrial; }
  else r = scene_find<true>(a.rowptr, a.r0, a.r1, i + a.rowptr[a.r0] + a.r0);
  int const c = a.tcopy0[r];
  if (c <= 0) return;                                       // a ray without state elements belongs to no slice
  long const s = (long)(c - 1) / a.per;
  a.flag[t * a.nslice + s] = 1;
}

// The fold of the flags into what the loop and the policy read, workgroup g striding over the flags g * 256 + lane,
// + gridDim.x * 256, ...: a flagged trial of a slice that takes part gets cost NaN (trial passes, cost given); a flagged
// slice that is active becomes JUR_RET_FAILED (Jacobian, reuse and gradient passes: before the solve, which then skips it
// as every later kernel does).  A lane reads and writes the state of its own slice only.  part[g]: how many cells the
// workgroup changed, a fixed tree over its lanes in LDS; the host adds the parts.
__global__ __launch_bounds__(256) void jur_scene_overflow_fold_kernel(jur_scene_ovfold_t a) {
  __shared__ long cnt[256];
  long const n = a.cost ? a.nslice * a.ntrial : a.nslice;
  long c = 0;
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < n; g += (long)gridDim.x * 256) {
    if (!a.flag[g]) continue;
    long const s = a.cost ? g - (g / a.nslice) * a.nslice : g;
    if (a.state && a.state[s] != 0) continue;
    if (a.cost) a.cost[g] = __builtin_nan("");
    else a.state[s] = JUR_RET_FAILED;
    c++;
  }
  cnt[threadIdx.x] = c;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) cnt[threadIdx.x] += cnt[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.part[blockIdx.x] = cnt[0];
}

}  // namespace

extern "C" int jurk_prepare_atm(jur_view_t const *v, double *d_pslope, void *stream) {
  int const block = 256;
  hipLaunchKernelGGL(jur_pslope_kernel, dim3((v->atm_np + block - 1) / block), dim3(block), 0, (hipStream_t)stream,
                     v->atm_np, v->atm_z, v->atm_p, d_pslope);
  return (int)hipGetLastError();
}

// ---- full a-priori precision of the slices (jur_model_set_prior_precision) -------------------------------------------
// P = R + diag(r); of R only the diagonal and the lower triangle are read (R_ij from R[max][min]).  These kernels form
// what the solve, inverse and product kernels above then work on unchanged.  No atomics, no waits between workgroups,
// every chain fixed by w alone.
//
// Assembly, one wavefront per row i of system s: D_j = A_jj + (R_jj + r_j) decides who is live; M_ij = A_ij + P_ij for
// j <= i between live elements (+0.0 in a dead row or column, so that the solve kernel finds D'_i = M_ii not > 0 there),
// then fma(lam, P_ij, M_ij) where lam is given (JUR_DAMP_PRIOR: a live D' stays > 0 since P_ii >= 0); g_i = fma(r_i, d_i,
// b_i) + (R d)_i with (R d)_i over the live j: lane l takes j = l, l + 64, ... ascending as a chain of fused multiply-adds,
// then the fixed tree of jur_scene_diag_rows_kernel runs over the 64 lanes.  With R = 0 that is the solve kernel's own g.
// Without A (the P of the smoothing error) nothing is masked.  No LDS, no barrier.
__global__ __launch_bounds__(256) void jur_scene_prior_assemble_kernel(jur_scene_pasm_t a) {
  long const nb = a.wptr[a.nslice], e = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= nb) return;                                      // (uniform in the wavefront)
  int const lane = threadIdx.x & 63;
  long const s = scene_find<false>(a.wptr, 0, a.nslice, e);
  if (a.state && a.state[s] != 0) return;                   // (uniform in the wavefront)
  int const w = (int)(a.wptr[s + 1] - a.wptr[s]), i = (int)(e - a.wptr[s]);
  double const *const A = a.A ? a.A + a.aptr[s] : nullptr, *const R = a.R + a.aptr[s], *const r = a.ivar + a.wptr[s];
  double const *const d = a.b ? a.d + a.wptr[s] : nullptr;
  double *const M = a.M + a.aptr[s];
  double const lam = a.lam ? a.lam[s] : 0.;
  double const Pii = R[(long)i * w + i] + r[i];
  bool const li = !A || A[(long)i * w + i] + Pii > 0;
  double acc = 0.;
  for (int j = lane; j < w; j += 64) {
    double const Rij = j <= i ? R[(long)i * w + j] : R[(long)j * w + i];
    bool lj = li;
    if (A && j != i) lj = A[(long)j * w + j] + (R[(long)j * w + j] + r[j]) > 0;
    if (d && lj) acc = fma(Rij, d[j], acc);
    if (j <= i) {
      double const Pij = j == i ? Pii : Rij;
      double v = 0.;
      if (li && lj) {
        v = A ? A[(long)i * w + j] + Pij : Pij;
        if (a.lam) v = fma(lam, Pij, v);
      }
      M[(long)i * w + j] = v;
    }
  }
  if (!d) return;
  for (int h = 32; h > 0; h >>= 1) acc += __shfl_down(acc, h, 64);
  if (lane == 0) a.g[e] = li ? fma(r[i], d[i], a.b[e]) + acc : 0.;
}

// v^T R v of one system by a workgroup of four wavefronts: wavefront k takes the rows i = k, k + 4, ... ascending, each row
// as in the assembly (lanes j = l, l + 64, ..., then the tree), q_k = fma(v_i, (R v)_i, q_k); then (q_0 + q_1) + (q_2 + q_3).
__device__ inline double scene_prior_quad(double const *__restrict__ R, double const *__restrict__ v, int w, double *part) {
  int const wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double q = 0.;
  for (int i = wave; i < w; i += 4) {
    double acc = 0.;
    for (int j = lane; j < w; j += 64) acc = fma(j <= i ? R[(long)i * w + j] : R[(long)j * w + i], v[j], acc);
    for (int h = 32; h > 0; h >>= 1) acc += __shfl_down(acc, h, 64);
    q = fma(v[i], acc, q);                                  // (lane 0 holds the row's sum)
  }
  if (lane == 0) part[wave] = q;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

// out[t][s] += v_t^T R_s v_t, one workgroup per (vector, system): the part of d^T P d that the diagonal chain of
// jur_scene_prior_kernel has not summed.  With R = 0 it adds +0.0.
__global__ __launch_bounds__(256) void jur_scene_prior_quad_kernel(jur_scene_pquad_t a) {
  __shared__ double part[4];
  long const g = blockIdx.x, t = g / a.nslice, s = g - t * a.nslice;
  int const w = (int)(a.wptr[s + 1] - a.wptr[s]);
  if (w <= 0 || (a.state && a.state[s] != 0)) return;       // (uniform)
  double const q = scene_prior_quad(a.R + a.aptr[s], a.v + t * a.wptr[a.nslice] + a.wptr[s], w, part);
  if (threadIdx.x == 0) a.out[g] = a.out[g] + q;
}

// pred of JUR_DAMP_PRIOR after the solve kernel has run on the assembled system with lam = 0: the sum over the live
// elements of dx_i fma(lam r_i, dx_i, g_i) in that kernel's order (every lane its elements ascending, then its tree over
// the 256 lanes) plus lam (dx^T R dx), a product and a sum rounded on their own.  A dead element's dx is +0.0 and R is
// finite: it adds exact zeros to the form.  A system that broke down keeps the 0 the solve kernel wrote.
__global__ __launch_bounds__(256) void jur_scene_prior_pred_kernel(jur_scene_pquad_t a) {
  __shared__ double red[256], part[4];
  long const s = blockIdx.x;
  int const tid = threadIdx.x, w = (int)(a.wptr[s + 1] - a.wptr[s]);
  if (w <= 0 || (a.state && a.state[s] != 0) || a.status[s] != 0) return;   // (uniform)
  double const *const dx = a.v + a.wptr[s], *const r = a.ivar + a.wptr[s], *const gg = a.g + a.wptr[s], *const lv = a.live + a.wptr[s];
  double const lam = a.lam[s];
  double sum = 0.;
  for (int i = tid; i < w; i += 256)
    if (lv[i] > 0) sum += dx[i] * fma(lam * r[i], dx[i], gg[i]);
  red[tid] = sum;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  double const q = scene_prior_quad(a.R + a.aptr[s], dx, w, part);
  if (tid == 0) a.out[s] = red[0] + lam * q;
}

// d[t][e] = xa_e - (x_e + dx[t][e]), the difference jur_scene_prior_kernel forms (of the bounded sum where a box is set),
// one lane per trial and element
__global__ __launch_bounds__(256) void jur_scene_prior_diff_kernel(jur_scene_trial_t a) {
  long const g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long const nb = a.wptr[a.nslice];
  if (g >= (a.dx ? nb * a.ntrial : nb)) return;
  long const e = g % nb;
  long const s = scene_find<false>(a.wptr, 0, a.nslice, e);
  if (a.state && a.state[s] != 0) return;
  double x = a.base[(long)a.erow[e] * a.np0 + a.eip[e]];
  if (a.dx) {
    x = x + a.dx[g];
    if (a.lo) JUR_STATE_BOUND(x, x, a.lo[e], a.hi[e]);
  }
  a.out[g] = a.xa[e] - x;
}

// sigma_smooth_i = sqrt(max(sum_j (S P)_ij S_ij, 0)), one wavefront per row as jur_scene_diag_rows_kernel's noise sum
// (a.avk holds S P here; the rows of dead elements and of a system that broke down are +0.0 there)
__global__ __launch_bounds__(256) void jur_scene_prior_smooth_kernel(jur_scene_diag_t a) {
  long const nb = a.wptr[a.nslice], e = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= nb) return;                                      // (uniform in the wavefront)
  int const lane = threadIdx.x & 63;
  long const s = scene_find<false>(a.wptr, 0, a.nslice, e);
  int const w = (int)(a.wptr[s + 1] - a.wptr[s]), i = (int)(e - a.wptr[s]);
  double const *const Si = a.S + a.aptr[s] + (long)i * w, *const Ki = a.avk + a.aptr[s] + (long)i * w;
  double smooth = 0.;
  for (int j = lane; j < w; j += 64) smooth = fma(Ki[j], Si[j], smooth);
  for (int h = 32; h > 0; h >>= 1) smooth += __shfl_down(smooth, h, 64);
  if (lane == 0) a.sigma_smooth[e] = sqrt(smooth > 0 ? smooth : 0.);
}

// Sa of jur_prior_corr_host, one lane per entry (i, j <= i) of a system, mirrored: sigma_i^2 on the diagonal; within a
// quantity q with cz[q] > 0 the product (sigma_i sigma_j) exp(-(|z_i - z_j| / cz[q])), every operation rounded on its own;
// +0.0 elsewhere.
__global__ __launch_bounds__(256) void jur_scene_prior_cov_kernel(jur_scene_pcov_t a) {
  long const g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= a.aptr[a.nslice]) return;
  long const s = scene_find<false>(a.aptr, 0, a.nslice, g);
  long const w = a.wptr[s + 1] - a.wptr[s], i = (g - a.aptr[s]) / w, j = (g - a.aptr[s]) - i * w;
  if (j > i) return;
  long const ei = a.wptr[s] + i, ej = a.wptr[s] + j;
  double v = 0.;
  if (i == j) v = a.sigma[ei] * a.sigma[ei];
  else if (a.iq[ei] == a.iq[ej]) {
    double const c = a.cz[a.iq[ei]];
    if (c > 0) v = (a.sigma[ei] * a.sigma[ej]) * exp(-(fabs(a.z[ei] - a.z[ej]) / c));
  }
  double *const Sa = a.Sa + a.aptr[s];
  Sa[i * w + j] = v;
  if (i > j) Sa[j * w + i] = v;
}

static unsigned scene_grid(long lanes) { return (unsigned)((lanes + 255) / 256); }

extern "C" int jurk_scene_stack(jur_scene_stack_t const *a, void *stream) {
  if (a->nt <= 0) return 0;
  hipLaunchKernelGGL(jur_scene_stack_kernel, dim3(scene_grid(a->nt)), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int jurk_scene_hydro(jur_scene_hydro_t const *a, void *stream) {
  if (a->nseg <= 0) return 0;
  hipLaunchKernelGGL(jur_scene_hydro_kernel, dim3((unsigned)a->nseg), dim3(64), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int jurk_scene_rays(jur_scene_pass_t const *a, void *stream) {
  if (a->n <= 0) return 0;
  hipLaunchKernelGGL(jur_scene_rays_kernel, dim3(scene_grid(a->n)), dim3(256), 0, (hipStream_t)stream, *a);
  hipLaunchKernelGGL(jur_scene_mask_kernel, dim3(scene_grid(a->n * a->nd)), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

// (rowptr is device memory: the host passes the number of block elements of the pass)
extern "C" int jurk_scene_quot(jur_scene_pass_t const *a, long nk, void *stream) {
  if (nk > 0) hipLaunchKernelGGL(jur_scene_quot_kernel, dim3(scene_grid(nk)), dim3(256), 0, (hipStream_t)stream, *a);
  if (a->r1 > a->r0)
    hipLaunchKernelGGL(jur_scene_gather_kernel, dim3(scene_grid((a->r1 - a->r0) * a->nd)), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int jurk_scene_fov(jur_scene_fov_t const *a, void *stream) {
  if (a->r1 <= a->r0 || a->n < 1) return 0;
  hipLaunchKernelGGL(jur_scene_fov_kernel, dim3((unsigned)(a->r1 - a->r0)), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

// (the tile counts are the host's: ntiles = tptr[nslice])
extern "C" int jurk_scene_normal(jur_scene_pass_t const *a, jur_scene_normal_t const *n, long ntiles, void *stream) {
  if (ntiles <= 0 || a->r1 <= a->r0) return 0;
  hipLaunchKernelGGL(jur_scene_normal_kernel, dim3((unsigned)ntiles), dim3(256), 0, (hipStream_t)stream, *a, *n);
  return (int)hipGetLastError();
}

// (the workgroup counts are the host's: ngroups = gptr[nslice])
extern "C" int jurk_scene_gradient(jur_scene_pass_t const *a, jur_scene_normal_t const *n, jur_scene_grad_t const *g, long ngroups, void *stream) {
  if (ngroups <= 0 || a->r1 <= a->r0) return 0;
  hipLaunchKernelGGL(jur_scene_gradient_kernel, dim3((unsigned)ngroups), dim3(256), 0, (hipStream_t)stream, *a, *n, *g);
  return (int)hipGetLastError();
}

// (one damping per launch: a->lam, a->dx, a->pred, a->status are that damping's)
extern "C" int jurk_scene_solve(jur_scene_solve_t const *a, void *stream) {
  if (a->nslice <= 0) return 0;
  hipLaunchKernelGGL(jur_scene_solve_kernel, dim3((unsigned)a->nslice), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

// (the maps and wptr are device memory: the host passes the block counts and nb = wptr[nslice])
extern "C" int jurk_scene_diag(jur_scene_diag_t const *a, long ninv, long ntile, long nb, void *stream) {
  if (a->nslice <= 0) return 0;
  hipStream_t const s = (hipStream_t)stream;
  if (ninv > 0) hipLaunchKernelGGL(jur_scene_inverse_kernel, dim3((unsigned)ninv), dim3(256), 0, s, *a);
  if (ntile > 0) hipLaunchKernelGGL(jur_scene_avk_kernel, dim3((unsigned)ntile), dim3(256), 0, s, *a);
  if (nb > 0) hipLaunchKernelGGL(jur_scene_diag_rows_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(jur_scene_dofs_kernel, dim3((unsigned)a->nslice), dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}

extern "C" int jurk_scene_weff(jur_scene_weff_t const *a, void *stream) {
  if (a->n <= 0) return 0;
  hipLaunchKernelGGL(jur_scene_weff_kernel, dim3(scene_grid(a->n)), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

// (the tile and workgroup counts are the host's: jur_gain_maps and gptr[nslice]; the budget only with components)
extern "C" int jurk_scene_gain(jur_scene_gain_t const *a, long ntile, long ngroups, void *stream) {
  hipStream_t const s = (hipStream_t)stream;
  if (ntile > 0) hipLaunchKernelGGL(jur_scene_gain_kernel, dim3((unsigned)ntile), dim3(256), 0, s, *a);
  if (a->ncomp > 0 && ngroups > 0) hipLaunchKernelGGL(jur_scene_budget_kernel, dim3((unsigned)ngroups), dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}

// (the tile and workgroup counts are the host's: jur_param_maps and pptr[nslice]; the quadratic forms only with components)
extern "C" int jurk_scene_cross_pass(jur_scene_param_t const *a, int const *pmap, long ntile, long kb0, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (ntile > 0) hipLaunchKernelGGL(jur_scene_cross_pass_kernel, dim3((unsigned)ntile), dim3(256), 0, s, *a, pmap, kb0);
  return (int)hipGetLastError();
}

extern "C" int jurk_scene_param(jur_scene_param_t const *a, long ntile, long ngroups, void *stream) {
  hipStream_t const s = (hipStream_t)stream;
  if (ntile > 0) hipLaunchKernelGGL(jur_scene_cross_kernel, dim3((unsigned)ntile), dim3(256), 0, s, *a);
  if (a->nvar + a->ncov > 0 && ngroups > 0) hipLaunchKernelGGL(jur_scene_param_kernel, dim3((unsigned)ngroups), dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}

// (wptr is device memory: the host passes the number of state elements nb = wptr[nslice])
extern "C" int jurk_scene_elements(jur_scene_trial_t const *a, int op, long nb, void *stream) {
  long const lanes = op == JUR_ELEM_APPLY ? nb * a->ntrial : nb;
  if (lanes <= 0) return 0;
  hipLaunchKernelGGL(jur_scene_elements_kernel, dim3(scene_grid(lanes)), dim3(256), 0, (hipStream_t)stream, *a, op);
  return (int)hipGetLastError();
}

extern "C" int jurk_scene_prior(jur_scene_trial_t const *a, void *stream) {
  long const lanes = a->nslice * (a->dx ? a->ntrial : 1);
  if (lanes <= 0) return 0;
  hipLaunchKernelGGL(jur_scene_prior_kernel, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int jurk_scene_trial_rays(jur_scene_trial_pass_t const *a, void *stream) {
  if (a->n <= 0) return 0;
  hipLaunchKernelGGL(jur_scene_trial_rays_kernel, dim3(scene_grid(a->n)), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int jurk_scene_trial_cost(jur_scene_trial_pass_t const *a, void *stream) {
  if (a->nslice <= 0 || a->r1 <= a->r0) return 0;
  hipLaunchKernelGGL(jur_scene_trial_cost_kernel, dim3((unsigned)(a->nslice * a->ntrial)), dim3(64), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int jurk_scene_compact(jur_scene_compact_t const *a, void *stream) {
  if (a->n <= 0) return 0;
  hipLaunchKernelGGL(jur_scene_compact_kernel, dim3(scene_grid(a->n)), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int jurk_scene_overflow(jur_scene_ovf_t const *a, void *stream) {
  if (a->n <= 0 || a->nslice <= 0) return 0;
  hipLaunchKernelGGL(jur_scene_overflow_kernel, dim3(scene_grid(a->n)), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int jurk_scene_overflow_fold(jur_scene_ovfold_t const *a, void *stream) {
  long const lanes = a->cost ? a->nslice * a->ntrial : a->nslice;
  if (lanes <= 0) return 0;
  hipLaunchKernelGGL(jur_scene_overflow_fold_kernel, dim3((unsigned)jur_scene_overflow_parts(lanes)), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

// (wptr is device memory: the host passes nb = wptr[nslice], the number of rows)
extern "C" int jurk_scene_prior_assemble(jur_scene_pasm_t const *a, long nb, void *stream) {
  if (nb <= 0) return 0;
  hipLaunchKernelGGL(jur_scene_prior_assemble_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int jurk_scene_prior_quad(jur_scene_pquad_t const *a, void *stream) {
  if (a->nslice <= 0 || a->nvec <= 0) return 0;
  hipLaunchKernelGGL(jur_scene_prior_quad_kernel, dim3((unsigned)(a->nslice * a->nvec)), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int jurk_scene_prior_pred(jur_scene_pquad_t const *a, void *stream) {
  if (a->nslice <= 0) return 0;
  hipLaunchKernelGGL(jur_scene_prior_pred_kernel, dim3((unsigned)a->nslice), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int jurk_scene_prior_diff(jur_scene_trial_t const *a, long nb, void *stream) {
  long const lanes = a->dx ? nb * a->ntrial : nb;
  if (lanes <= 0) return 0;
  hipLaunchKernelGGL(jur_scene_prior_diff_kernel, dim3(scene_grid(lanes)), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

// (S P by the product kernel as it stands, then the row sums)
extern "C" int jurk_scene_prior_smooth(jur_scene_diag_t const *a, long ntile, long nb, void *stream) {
  if (a->nslice <= 0 || nb <= 0) return 0;
  hipStream_t const s = (hipStream_t)stream;
  if (ntile > 0) hipLaunchKernelGGL(jur_scene_avk_kernel, dim3((unsigned)ntile), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(jur_scene_prior_smooth_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}

// (the inverse of jur_prior_corr_host: the inverse kernel alone, after jurk_scene_solve has left the factor)
extern "C" int jurk_scene_prior_inverse(jur_scene_diag_t const *a, long ninv, void *stream) {
  if (a->nslice <= 0 || ninv <= 0) return 0;
  hipLaunchKernelGGL(jur_scene_inverse_kernel, dim3((unsigned)ninv), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int jurk_scene_prior_cov(jur_scene_pcov_t const *a, long na, void *stream) {
  if (na <= 0) return 0;
  hipLaunchKernelGGL(jur_scene_prior_cov_kernel, dim3(scene_grid(na)), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

static int g_trace_lanes = 0;          // 0: by launch size
extern "C" void jurk_tune_trace(int lanes) { g_trace_lanes = (lanes == 1 || lanes == 4) ? lanes : 0; }
static int g_trace_slice = 0;          // 0: by launch (see jurk_launch_trace), 1: never, 2: wherever the slice fits
extern "C" void jurk_tune_trace_slice(int mode) { g_trace_slice = (mode == 1 || mode == 2) ? mode : 0; }
// room for the slice's rows beside the four wavefronts' tangent-point columns: 4 x 7680 B + 10 240 B = 40 KiB, a
// quarter of the CU's LDS
#ifndef JUR_TRACE_SLAB_DOUBLES
#define JUR_TRACE_SLAB_DOUBLES 1280
#endif

extern "C" int jurk_cloud_lds_points(void) { return JUR_CLOUD_LDS_POINTS; }

extern "C" int jurk_kat_cloud_mean(jur_view_t const *v, jur_cloud_t const *cld, long n, int a0, int len, double const *z0,
                                   double const *lat0, double const *x0, double *out, void *stream) {
  // (the kernel indexes the rows and the table by a0 .. a0 + len - 1)
  if (n < 1 || a0 < 0 || len < 1 || (long)a0 + len > v->atm_np || !cld || cld->np != v->atm_np || !cld->x1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(jur_kat_cloud_mean_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *v, *cld, n, a0,
                     len, z0, lat0, x0, out);
  return (int)hipGetLastError();
}

extern "C" int jurk_launch_trace(jur_view_t const *v, jur_track_t const *trk, jur_cloud_t const *cld, jur_chunk_t const *c, void *stream) {
  if (c->n <= 0) return 0;
  if (trk && trk->ip == 3) {             // the 3-D rule has one instance too; its table holds a position per atmosphere point
    if (!cld || !cld->x1 || cld->np != v->atm_np || cld->np < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(jur_cloud_trace_kernel, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *v, *c, *cld);
    return (int)hipGetLastError();
  }
  if (trk && trk->ip == 2) {             // the 2-D rule has one instance: a lane per ray, workgroups of 256 slots
    if (trk->nprof < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(jur_track_trace_kernel, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *v, *c, *trk);
    return (int)hipGetLastError();
  }
  int const block = 64;
  // a quad of lanes per ray where the launch stays within the chip's 4096 tracer wavefront slots with it AND the rays
  // have several emitters' columns to share (see jur_trace_lanes_kernel)
  static int const env_lanes = getenv("JUR_TRACE_LANES") ? atoi(getenv("JUR_TRACE_LANES")) : 0;     // A/B switch, read once
  int const forced = g_trace_lanes ? g_trace_lanes : env_lanes;
  int const lanes = forced == 1 || forced == 4 ? forced : ((c->n <= 65536 && v->ng >= 3) ? 4 : 1);
  // The profile slice in LDS (jur_trace_slice_kernel) where a lane traces a ray and the longest slice fits the slab: four
  // workgroups of 4 x 7680 B of tangent-point columns + slab share the CU's 160 KiB, as the sixteen wavefronts of
  // jur_trace_kernel do.  By itself only for launches that are sorted by slice (else most workgroups straddle two) and
  // fill the chip's 4096 tracer wavefront slots: below that a workgroup of four tiles spreads the rays over fewer CUs.
  static int const env_slice = getenv("JUR_TRACE_SLICE") ? atoi(getenv("JUR_TRACE_SLICE")) : 0;     // A/B switch, read once
  int const mode = g_trace_slice ? g_trace_slice : (env_slice == 1 || env_slice == 2) ? env_slice : 0;
  long const slab = (long)(4 + v->ng + v->nw) * v->atm_maxslice;
  bool const fits = v->atm_maxslice >= 2 && slab <= JUR_TRACE_SLAB_DOUBLES;
  if (lanes == 1 && fits && mode != 1 && (mode == 2 || (c->slice_sorted && c->n >= 4096 * 64))) {
    int const wg = 64 * JUR_TRACE_SLICE_WAVES;
    size_t const lds = 8 * (size_t)(JUR_TRACE_SLICE_WAVES * 15 * 64 + slab);
    jur_chunk_t cs = *c;
    if (wg > 256) cs.blk_order = NULL;
    // with a block order the grid covers whole blocks of 256 slots: any block may come last
    unsigned const grid = cs.blk_order ? (unsigned)((c->n + 255) / 256) * (256 / wg) : (unsigned)((c->n + wg - 1) / wg);
    hipLaunchKernelGGL(jur_trace_slice_kernel, dim3(grid), dim3(wg), lds, (hipStream_t)stream, *v, cs, (int)slab);
    return (int)hipGetLastError();
  }
  int const grid = (lanes == 1 && c->blk_order) ? (c->n + 255) / 256 * 4 : (int)(((long)c->n * lanes + block - 1) / block);
  if (lanes == 4) hipLaunchKernelGGL(jur_trace_lanes_kernel<4>, dim3(grid), dim3(block), 0, (hipStream_t)stream, *v, *c);
  else hipLaunchKernelGGL(jur_trace_kernel, dim3(grid), dim3(block), 0, (hipStream_t)stream, *v, *c);
  return (int)hipGetLastError();
}

// dynamic LDS beyond 64 KB needs the attribute once per kernel AND per device (models may live on several GPUs of one
// process, their lanes launch from several threads); `raised` holds one bit per device for the caller's kernel set
static int raise_lds_limit(std::mutex &mu, unsigned long long &raised, void const *const *funcs, int nfunc, bool needed) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return (int)hipErrorInvalidDevice;
  std::lock_guard<std::mutex> lock(mu);
  if ((raised >> dev) & 1ull) return 0;
  hipError_t e = hipSuccess;
  for (int i = 0; i < nfunc && e == hipSuccess; i++) e = hipFuncSetAttribute(funcs[i], hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
  if (e != hipSuccess) { (void)hipGetLastError(); return needed ? (int)e : 0; }
  raised |= 1ull << dev;
  return 0;
}

// cga != 0: the model runs FORMOD 1 -- jur_cga_kernel in the variant the same rules choose (the switch stays on the
// host: jur_view_t is an argument of every kernel)
extern "C" int jurk_launch_ega(jur_view_t const *v, jur_chunk_t const *c, int cga, void *stream) {
  if (c->n <= 0 || v->ng <= 0) return 0;
  int const block = 256;   // (128 rays per workgroup: 34.6 against 33.7 ms; 64: the staged descriptors limit the occupancy, 45 ms)
  int const nrb = (c->n + block - 1) / block, npair = v->nd * v->ng;
  unsigned const grid = xcd_grid(nrb, npair);
  hipStream_t s = (hipStream_t)stream;
  // LDS copy of one pair's descriptors per workgroup: 16 B x (levels + curves of the largest pair)
  // (+ 8 B x the same counts for the reciprocal bracket widths of strictly increasing tables)
  size_t const lds = (sizeof(jur_lvl_t) + 8) * JUR_TBLNP + (sizeof(jur_crv_t) + 8) * (size_t)v->max_pair_curves;
  bool const use_lds = v->max_pair_curves > 0 && lds <= 48 * 1024;
  bool const rcpb = use_lds && v->fast_arith;
  if (cga) {
    if (v->sorted_tables) {
      if (rcpb) hipLaunchKernelGGL((jur_cga_kernel<true, true, true>), dim3(grid), dim3(block), lds, s, *v, *c, nrb);
      else if (use_lds) hipLaunchKernelGGL((jur_cga_kernel<true, true, false>), dim3(grid), dim3(block), lds, s, *v, *c, nrb);
      else hipLaunchKernelGGL((jur_cga_kernel<true, false, false>), dim3(grid), dim3(block), 0, s, *v, *c, nrb);
    } else {
      if (use_lds) hipLaunchKernelGGL((jur_cga_kernel<false, true, false>), dim3(grid), dim3(block), lds, s, *v, *c, nrb);
      else hipLaunchKernelGGL((jur_cga_kernel<false, false, false>), dim3(grid), dim3(block), 0, s, *v, *c, nrb);
    }
    return (int)hipGetLastError();
  }
  if (v->sorted_tables) {
    if (rcpb) hipLaunchKernelGGL((jur_ega_kernel<true, true, true>), dim3(grid), dim3(block), lds, s, *v, *c, nrb);
    else if (use_lds) hipLaunchKernelGGL((jur_ega_kernel<true, true, false>), dim3(grid), dim3(block), lds, s, *v, *c, nrb);
    else hipLaunchKernelGGL((jur_ega_kernel<true, false, false>), dim3(grid), dim3(block), 0, s, *v, *c, nrb);
  } else {
    if (use_lds) hipLaunchKernelGGL((jur_ega_kernel<false, true, false>), dim3(grid), dim3(block), lds, s, *v, *c, nrb);
    else hipLaunchKernelGGL((jur_ega_kernel<false, false, false>), dim3(grid), dim3(block), 0, s, *v, *c, nrb);
  }
  return (int)hipGetLastError();
}

// how jur_combine runs: channels per workgroup (0: always one channel per workgroup), segments between barriers,
// smallest launch (rays x channels) that takes the grouped kernel
static int g_combine_group = -1, g_combine_sync = 8, g_combine_forced = 0;
static long g_combine_min_lanes = 1000000L;
extern "C" void jurk_tune_combine(int group, int sync, long min_lanes) {
  g_combine_forced = group >= 0;                 // < 0: back to the defaults and the default rule
  g_combine_group = group < 0 ? 4 : (group > 6 ? 6 : group);   // 6 source-function tables fill the 64 KB of LDS a launch may ask for
  g_combine_sync = sync;
  g_combine_min_lanes = min_lanes;
}

extern "C" int jurk_launch_combine(jur_view_t const *v, jur_chunk_t const *c, void *stream) {
  if (c->n <= 0) return 0;
  int const block = 256;
  int const nrb = (c->n + block - 1) / block;
  unsigned const grid = xcd_grid(nrb, v->nd);
  static std::once_flag env_once;                  // first launch: the environment may override the defaults (A/B
  std::call_once(env_once, [] {                    // switch); once, whichever lane's thread comes first
    if (g_combine_group >= 0) return;              // jur_tune_combine has spoken already
    g_combine_group = getenv("JUR_COMBINE_GROUP") ? atoi(getenv("JUR_COMBINE_GROUP")) : 4;
    g_combine_forced = getenv("JUR_COMBINE_GROUP") != NULL;
    if (g_combine_group > 6) g_combine_group = 6;
    if (getenv("JUR_COMBINE_SYNC")) g_combine_sync = atoi(getenv("JUR_COMBINE_SYNC"));
    if (getenv("JUR_COMBINE_MIN_LANES")) g_combine_min_lanes = atol(getenv("JUR_COMBINE_MIN_LANES"));
  });
  if (g_combine_group < 0) g_combine_group = 4;
  int const group = g_combine_group, sync = g_combine_sync;
  // grouped only when the launch fills the chip several times over -- below that a call is as long as its longest
  // chain, and barriers between wavefronts lengthen it (nadir_1e5, 3e5 lanes: 0.66 against 0.37 ms) -- and, by
  // default, only when the channels fall into full groups of four: groups of two or three and ragged last groups were
  // measured slower than one channel per workgroup (tools/bench_combine_groups.py: 2 channels +7 %, 3 +17 %,
  // 6 = 4 + 2 +27 %).  A group size set through jur_tune_combine / JUR_COMBINE_GROUP is taken as it is.
  // (with many channels the one ragged group at the end does not matter: 2378 = 594 x 4 + 2)
  bool const fits = g_combine_forced || (group == 4 && (v->nd % 4 == 0 || v->nd >= 64));
  if (group > 0 && v->nd > 1 && fits && (long)c->n * v->nd >= g_combine_min_lanes) {
    int const CG = v->nd < group ? v->nd : group, SUB = 8 / CG, W = CG * SUB;
    jur_chunk_t cs = *c;
    if (SUB > 4) cs.blk_order = NULL;              // super-blocks of 512 slots: wider than the blocks of the order
    // (with a block order the grid covers whole blocks of 256 slots: any block may come last)
    int const nsb = cs.blk_order ? (c->n + 255) / 256 * (4 / SUB) : (c->n + SUB * 64 - 1) / (SUB * 64), ncg = (v->nd + CG - 1) / CG;
    unsigned const g2 = xcd_grid(nsb, ncg);
    int mask = -1;                                 // barrier every 2^k segments, k from JUR_COMBINE_SYNC (<= 0: none)
    if (sync > 0) { mask = 1; while (mask * 2 <= sync) mask *= 2; mask -= 1; }
    hipLaunchKernelGGL(jur_combine_group_kernel, dim3(g2), dim3(64 * W), sizeof(double) * (JUR_TBLNS * CG + 2 + 64), (hipStream_t)stream,
                       *v, cs, nsb, CG, mask);
    return (int)hipGetLastError();
  }
  hipLaunchKernelGGL(jur_combine_kernel, dim3(grid), dim3(block), sizeof(double) * (JUR_TBLNS + 64), (hipStream_t)stream, *v, *c,
                     nrb);
  return (int)hipGetLastError();
}

extern "C" int jurk_launch_contrib(jur_view_t const *v, jur_chunk_t const *c, long nr, double *rad_c, double *tau_c, void *stream) {
  if (c->n <= 0) return 0;
  int const block = 256;
  int const nrb = (c->n + block - 1) / block;
  long const nitem = (long)v->nd * (v->ng + 1);
  if (((long)(nrb >> 3) + 1) * 8 * nitem * block >= (1L << 32)) return (int)hipErrorInvalidValue;   // (xcd_grid <= that)
  unsigned const grid = xcd_grid(nrb, (int)nitem);
  hipLaunchKernelGGL(jur_contrib_kernel, dim3(grid), dim3(block), sizeof(double) * (JUR_TBLNS + 64), (hipStream_t)stream, *v, *c,
                     nrb, nr, rad_c, tau_c);
  return (int)hipGetLastError();
}

extern "C" int jurk_launch_kquot(long nq, long n, double const *d_rad, double const *d_h, double *d_kq, void *stream) {
  if (nq <= 0 || n <= 0) return 0;
  hipLaunchKernelGGL(jur_kquot_kernel, dim3((unsigned)((nq * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nq, n, nq, d_rad, d_h, d_kq);
  return (int)hipGetLastError();
}

extern "C" int jurk_tile_max(int n, int const *d_np, int *d_tile_np, void *stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(jur_tilemax_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, d_np, d_tile_np);
  return (int)hipGetLastError();
}

extern "C" int jurk_launch_cg(jur_view_t const *v, jur_chunk_t const *c, double *cgp, double *cgt, double *cgu,
                              void *stream) {
  if (c->n <= 0 || v->ng <= 0) return 0;
  int const block = 256;                                   // 4 pencils per workgroup
  long const pencils = (long)c->n * v->ng;
  unsigned const grid = (unsigned)((pencils * 64 + block - 1) / block);
  hipLaunchKernelGGL(jur_cg_kernel, dim3(grid), dim3(block), 0, (hipStream_t)stream, *v, *c, cgp, cgt, cgu);
  return (int)hipGetLastError();
}

static size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

extern "C" long jurk_sort_tmp_bytes(long nr) {
  size_t cub = 0;
  if (hipcub::DeviceRadixSort::SortPairs(nullptr, cub, (unsigned long long const *)nullptr, (unsigned long long *)nullptr,
                                         (int const *)nullptr, (int *)nullptr, (int)nr) != hipSuccess)
    cub = 64 * (size_t)nr + (1 << 20);
  // ... and of the sort of the launch's blocks (jurk_block_order), which runs after it in the same scratch
  size_t cub_blk = 0;
  if (hipcub::DeviceRadixSort::SortPairs(nullptr, cub_blk, (unsigned const *)nullptr, (unsigned *)nullptr, (int const *)nullptr,
                                         (int *)nullptr, (int)((nr + 255) / 256)) != hipSuccess)
    cub_blk = cub;
  if (cub_blk > cub) cub = cub_blk;
  return (long)(2 * align_up(8 * (size_t)nr) + align_up(4 * (size_t)nr) + align_up(cub) + 256);
}

extern "C" int jurk_sort_rays(jur_view_t const *v, int by_profile, long nr, double const *d_geom, long ld, int *d_order, void *tmp,
                              long tmp_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  size_t const seg8 = align_up(8 * (size_t)nr), seg4 = align_up(4 * (size_t)nr);
  char *base = (char *)tmp;
  unsigned long long *key_in = (unsigned long long *)base, *key_out = (unsigned long long *)(base + seg8);
  int *id_in = (int *)(base + 2 * seg8);
  void *cub_tmp = base + 2 * seg8 + seg4;
  size_t cub_bytes = (size_t)tmp_bytes - 2 * seg8 - seg4;
  int const block = 256;
  hipLaunchKernelGGL(jur_raykey_kernel, dim3((unsigned)((nr + block - 1) / block)), dim3(block), 0, s, nr, ld, d_geom,
                     v->atm_time, v->atm_np, by_profile, key_in, id_in);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  e = hipcub::DeviceRadixSort::SortPairs(cub_tmp, cub_bytes, key_in, key_out, id_in, d_order, (int)nr, 0,
                                         by_profile ? 64 : 32, s);
  return (int)e;
}

// The order in which a launch over the sorted slots starts its blocks of 256: ascending tangent altitude of the block's
// lowest ray, so the longest paths first (see jur_chunk_t::blk_order).  Reads the sorted keys jurk_sort_rays has left in
// `tmp`; its own keys and ids lie where the ray sort's unsorted keys were.  The radix sort is stable: equal keys keep
// their blocks in ascending order, a permutation in any case.
extern "C" int jurk_block_order(long nr, int *d_blk_order, void *tmp, long tmp_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  size_t const seg8 = align_up(8 * (size_t)nr), seg4 = align_up(4 * (size_t)nr);
  int const nblk = (int)((nr + 255) / 256);
  size_t const seg = (4 * (size_t)nblk + 15) & ~(size_t)15;
  if (nr < 1 || 3 * seg > seg8) return (int)hipErrorInvalidValue;
  char *base = (char *)tmp;
  unsigned long long const *sorted_key = (unsigned long long const *)(base + seg8);
  unsigned *key_in = (unsigned *)base, *key_out = (unsigned *)(base + seg);
  int *id_in = (int *)(base + 2 * seg);
  void *cub_tmp = base + 2 * seg8 + seg4;
  size_t cub_bytes = (size_t)tmp_bytes - 2 * seg8 - seg4;
  hipLaunchKernelGGL(jur_blockkey_kernel, dim3((unsigned)((nblk + 3) / 4)), dim3(256), 0, s, nr, nblk, sorted_key, key_in, id_in);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  e = hipcub::DeviceRadixSort::SortPairs(cub_tmp, cub_bytes, key_in, key_out, id_in, d_blk_order, nblk, 0, 32, s);
  return (int)e;
}

// ---- known-answer hooks ----
// mode 0: the reference's bisections; 1: warm-started searches, descriptors from global memory; 2: ... from LDS;
// 3: LDS + reciprocal bracket widths (the variant the bench runs).  Returns hipErrorInvalidValue (1) when the
// tables do not admit the mode.
extern "C" int jurk_kat_ega(jur_view_t const *v, int g, int d, long n, double const *tau, double const *t, double const *u,
                            double const *p, int mode, int chain, double *out, void *stream) {
  if (n <= 0) return 0;
  size_t const lds = (sizeof(jur_lvl_t) + 8) * JUR_TBLNP + (sizeof(jur_crv_t) + 8) * (size_t)v->max_pair_curves;
  bool const lds_ok = v->max_pair_curves > 0 && lds <= 48 * 1024;
  if ((mode >= 1 && !v->sorted_tables) || (mode >= 2 && !lds_ok) || (mode == 3 && !v->strict_tables) || mode < 0 || mode > 3)
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  dim3 const grid(chain ? 1u : (unsigned)((n + 255) / 256)), block(256);
  if (mode == 0) {
    if (lds_ok) hipLaunchKernelGGL((jur_kat_ega_kernel<false, true, false>), grid, block, lds, s, *v, g, d, n, tau, t, u, p, chain, out);
    else hipLaunchKernelGGL((jur_kat_ega_kernel<false, false, false>), grid, block, 0, s, *v, g, d, n, tau, t, u, p, chain, out);
  } else if (mode == 1) hipLaunchKernelGGL((jur_kat_ega_kernel<true, false, false>), grid, block, 0, s, *v, g, d, n, tau, t, u, p, chain, out);
  else if (mode == 2) hipLaunchKernelGGL((jur_kat_ega_kernel<true, true, false>), grid, block, lds, s, *v, g, d, n, tau, t, u, p, chain, out);
  else hipLaunchKernelGGL((jur_kat_ega_kernel<true, true, true>), grid, block, lds, s, *v, g, d, n, tau, t, u, p, chain, out);   // what the batched kernel runs
  return (int)hipGetLastError();
}

// the same modes for the Curtis-Godson look-up (3: what jur_cga_kernel runs on strict tables)
extern "C" int jurk_kat_cga(jur_view_t const *v, int g, int d, long n, double const *tau, double const *t, double const *u,
                            double const *p, int mode, int chain, double *out, void *stream) {
  if (n <= 0) return 0;
  size_t const lds = (sizeof(jur_lvl_t) + 8) * JUR_TBLNP + (sizeof(jur_crv_t) + 8) * (size_t)v->max_pair_curves;
  bool const lds_ok = v->max_pair_curves > 0 && lds <= 48 * 1024;
  if ((mode >= 1 && !v->sorted_tables) || (mode >= 2 && !lds_ok) || (mode == 3 && !v->strict_tables) || mode < 0 || mode > 3)
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  dim3 const grid(chain ? 1u : (unsigned)((n + 255) / 256)), block(256);
  if (mode == 0) {
    if (lds_ok) hipLaunchKernelGGL((jur_kat_cga_kernel<false, true, false>), grid, block, lds, s, *v, g, d, n, tau, t, u, p, chain, out);
    else hipLaunchKernelGGL((jur_kat_cga_kernel<false, false, false>), grid, block, 0, s, *v, g, d, n, tau, t, u, p, chain, out);
  } else if (mode == 1) hipLaunchKernelGGL((jur_kat_cga_kernel<true, false, false>), grid, block, 0, s, *v, g, d, n, tau, t, u, p, chain, out);
  else if (mode == 2) hipLaunchKernelGGL((jur_kat_cga_kernel<true, true, false>), grid, block, lds, s, *v, g, d, n, tau, t, u, p, chain, out);
  else hipLaunchKernelGGL((jur_kat_cga_kernel<true, true, true>), grid, block, lds, s, *v, g, d, n, tau, t, u, p, chain, out);
  return (int)hipGetLastError();
}

extern "C" int jurk_kat_continua(jur_view_t const *v, int d, long n, double const *p, double const *t, double const *q,
                                 double const *u_co2, double const *u_h2o, double *out, void *stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(jur_kat_continua_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *v, d, n, p, t,
                     q, u_co2, u_h2o, out);
  return (int)hipGetLastError();
}

extern "C" int jurk_kat_update(jur_view_t const *v, int d, long n, int what, double const *a, double const *b, double const *c,
                               double *rad, double *tau, double *src, void *stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(jur_kat_update_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *v, d, n, what,
                     a, b, c, rad, tau, src);
  return (int)hipGetLastError();
}

extern "C" int jurk_kat_los(jur_view_t const *v, jur_chunk_t const *c, double *los, double *tsurf, void *stream) {
  if (c->n <= 0) return 0;
  long const n = (long)c->n * NLOS;
  hipLaunchKernelGGL(jur_kat_los_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *v, *c, los, tsurf);
  return (int)hipGetLastError();
}

// ---- fused kernel for small calls ----
// LDS bytes jur_pencil_kernel needs for RB rays per workgroup (0: the configuration does not fit)
extern "C" long jurk_pencil_lds_bytes(jur_view_t const *v, int RB) {
  long const bytes = 8 * pen_lds_doubles(v->nd, v->ng, v->nw, RB);
  return bytes <= 96 * 1024 ? bytes : 0;
}

// room for the profile slab: the longest slice of the atmosphere, if that stays inside 32 KB
static int pencil_atm_cap(jur_view_t const *v) {
  long const nrow = 7 + v->ng + v->nw;
  static int const off = getenv("JUR_PENCIL_NO_ATM_LDS") ? 1 : 0;      // A/B switch, read once
  if (!v->atm_sorted || v->atm_maxslice < 2 || off) return 0;
  return (nrow * v->atm_maxslice * 8 <= 32 * 1024) ? v->atm_maxslice : 0;
}

extern "C" int jurk_launch_pencil(jur_view_t const *v, jur_chunk_t const *c, int RB, void *stream) {
  if (c->n <= 0) return 0;
  long const lds = jurk_pencil_lds_bytes(v, RB);
  if (RB < 1 || RB > 64 || lds <= 0) return (int)hipErrorInvalidValue;
  int const npair = v->nd * v->ng;
  // up to 16 rays per workgroup the tracer wavefront has four lanes per ray (one refraction probe each) and, for
  // sorted tables, every chain four lanes (one corner curve each)
  static bool const no_quad = getenv("JUR_PENCIL_NO_QUAD") != nullptr;   // A/B switch, read once
  bool const quad = RB <= 16 && !no_quad;
  int NE = (RB * npair * ((quad && v->sorted_tables) ? 4 : 1) + 63) / 64, NC = (RB * v->nd + 63) / 64;
  NE = NE < 1 ? 1 : (NE > PEN_MAXE ? PEN_MAXE : NE);
  NC = NC < 1 ? 1 : (NC > PEN_MAXC ? PEN_MAXC : NC);
  dim3 const grid((unsigned)((c->n + RB - 1) / RB)), block((unsigned)(64 * (1 + NE + NC)));
  hipStream_t s = (hipStream_t)stream;
  int const atm_cap = pencil_atm_cap(v);
  long const lds_all = lds + 8L * (7 + v->ng + v->nw) * atm_cap;
  {
    static std::mutex mu;
    static unsigned long long raised = 0;                 // one bit per device, read and written under mu
    void const *const funcs[] = {reinterpret_cast<void const *>(&jur_pencil_kernel<true, true>), reinterpret_cast<void const *>(&jur_pencil_kernel<true, false>),
                                 reinterpret_cast<void const *>(&jur_pencil_kernel<false, true>), reinterpret_cast<void const *>(&jur_pencil_kernel<false, false>)};
    int const e = raise_lds_limit(mu, raised, funcs, 4, lds_all > 64 * 1024);
    if (e) return e;
  }
  if (v->sorted_tables) {
    if (quad) hipLaunchKernelGGL((jur_pencil_kernel<true, true>), grid, block, (size_t)lds_all, s, *v, *c, RB, NE, NC, atm_cap);
    else hipLaunchKernelGGL((jur_pencil_kernel<true, false>), grid, block, (size_t)lds_all, s, *v, *c, RB, NE, NC, atm_cap);
  } else {
    if (quad) hipLaunchKernelGGL((jur_pencil_kernel<false, true>), grid, block, (size_t)lds_all, s, *v, *c, RB, NE, NC, atm_cap);
    else hipLaunchKernelGGL((jur_pencil_kernel<false, false>), grid, block, (size_t)lds_all, s, *v, *c, RB, NE, NC, atm_cap);
  }
  return (int)hipGetLastError();
}

extern "C" int jurk_fill_records(jur_ue_t const *ue, jur_rec_t *rec, long long n, void *stream) {
  long long const nb = (n + 255) / 256;
  hipLaunchKernelGGL(jur_records_kernel, dim3((unsigned)(nb < 65536 ? (nb > 0 ? nb : 1) : 65536)), dim3(256), 0, (hipStream_t)stream, n, ue, rec);
  return (int)hipGetLastError();
}

extern "C" int jurk_launch_fov(long nr, int nd, double const *time, double const *vpz, double const *rad0, double const *tau0,
                               double *rad, double *tau, long ld, int n, double const *dz, double const *w, int *status, void *stream) {
  if (nr <= 0) return 0;
  long const total = nr * nd;
  hipLaunchKernelGGL(jur_fov_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nr, nd, time, vpz, rad0,
                     tau0, rad, tau, ld, n, dz, w, status);
  return (int)hipGetLastError();
}

extern "C" int jurk_launch_intpol(int ip, int ng, int nw, int ns, int nd_, int nx, double cx, double cz, double const *src,
                                  double const *x1, int const *idx, int const *nz, double const *dst, double const *x0, double *out,
                                  void *stream) {
  if (nd_ <= 0) return 0;
  IntpolArgs const a{ip, ng, nw, ns, nd_, nx, cx, cz, src, x1, idx, nz, dst, x0, out};
  hipLaunchKernelGGL(jur_intpol_kernel, dim3((unsigned)((nd_ + 127) / 128)), dim3(128), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
