/* jur_internal.h -- structures shared by the C host code and the HIP kernels.
 * Plain C so that gcc (host) and hipcc (device) agree on the layout. */
#ifndef JUR_INTERNAL_H
#define JUR_INTERNAL_H

#include <stdint.h>
#include "jurassic_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { int a, b; } jur_int2;
typedef struct { float u, eps; } jur_ue_t;
/* bracket [entry i, entry i+1] of a curve in one record: the two entries as stored and both slopes, formed on the
 * device once per model from the fp32 entries (strictly increasing tables only): what get_u and get_eps multiply with
 * instead of dividing by the bracket width */
typedef struct { float u0, e0, u1, e1; double du_de, de_du; } __attribute__((aligned(32))) jur_rec_t;
/* 16-byte descriptors: one load brings the axis value together with the extent
 * and the offset of the next level of the hierarchy. */
typedef struct { double p; int nt; int c0; } jur_lvl_t;   /* pressure level: nt curves from curve c0 */
typedef struct { double t; int nu; int e0; } jur_crv_t;   /* curve: nu (u,eps) entries from entry e0 OF ITS PAIR
                                                             (pair_e0[pair] + e0 in the ue array): 32 bits hold any
                                                             pair (<= 40 x 30 x 304 entries), the set may hold > 2^31 */

/* Everything about the continua that depends on the channel only, reduced on
 * the host once per model with the reference's own expression order
 * (jr_common.h:318-325, 336-357, 367-372, 381-386). */
typedef struct {
  double nu;
  double co2_cw296, co2_cw260, co2_cw230;   /* 2 cm^-1 grid interpolates            */
  double h2o_sc;                            /* sfac * cw296                         */
  double h2o_ratio;                         /* cw260 / cw296                        */
  double h2o_lnr_hi, h2o_lnr_lo;            /* ln(h2o_ratio) = hi + lo (from logl), for ratio^y = exp(y ln ratio) */
  double h2o_ctwfrn;                        /* cwfrn * fscal                        */
  double n2_b, n2_beta;
  double o2_b, o2_beta;
  int co2_on, h2o_on, n2_on, o2_on;         /* channel inside the continuum's range */
  int window;
  int pad;
} jur_chan_t;

/* LOS workspace: tiles of 64 ray slots, fields stored as [tile][point][field][64]. */
enum { JUR_F_P = 0, JUR_F_T = 1, JUR_F_DS = 2, JUR_F_QH2O = 3, JUR_F_K = 4 /* + nw, then u[ng] */ };

/* Read-only device view of a model; passed to kernels by value. */
typedef struct {
  int ng, nd, nw;
  int fourbit, ig_co2, ig_h2o;
  int refrac, write_bbt;
  double rayds, raydz;
  jur_chan_t const *chan;       /* [nd]                                         */
  double const *sr;             /* [nd][JUR_TBLNS] source function              */
  /* emissivity tables, CSR-like:
   * pair[g*nd+d] = {np, first level}; lvl per level; crv per curve;
   * ue = interleaved (u, eps) float pairs, unit stride along u. */
  jur_int2 const *pair;
  jur_lvl_t const *lvl;
  jur_crv_t const *crv;
  jur_ue_t const *ue;
  jur_rec_t const *rec;         /* [entries] bracket records (entries i, i+1 and the slopes of [i, i+1]), or NULL      */
  long long const *pair_e0;     /* [ng*nd] first entry of every pair in ue (64 bits: a full-extent many-channel set --
                                   2378 channels x 3 gases x 40 x 30 x 304 = 2.6e9 entries -- is addressed as
                                   wave-uniform pair base + 32-bit offset inside the pair)                        */
  int sorted_tables;            /* every axis and curve is non-decreasing: any bracket search
                                   finds what the reference's bisection finds                  */
  int atm_maxslice;             /* longest run of equal time stamps in the atmosphere          */
  int max_pair_curves;          /* most curves any (gas, channel) pair has (LDS staging size)  */
  int strict_tables;            /* sorted, and p, T axes and (as stored, fp32) all curves strictly increasing:
                                   no bracket of the look-up has zero width                                     */
  int fast_arith;               /* the look-up runs the strict-table arithmetic (JUR_ARITH_FAST on strict tables whose
                                   descriptors fit the LDS staging); 0: the reference's divisions operand for operand */
  /* atmosphere, compact SoA of atm_np points */
  int atm_np;
  int atm_sorted;               /* time stamps non-decreasing and z strictly monotone inside every slice */
  int atm_k_zero;               /* every atm_k[iw][ip] is +0.0 (all bits clear) on a sorted atmosphere: the tracer writes no
                                   extinction fields and their readers take 0.0 (jur_atm_k_zero; never set for rows
                                   the host has not seen)                                                         */
  double const *atm_time, *atm_z, *atm_lon, *atm_lat, *atm_p, *atm_t;
  double const *atm_q;          /* [ng][atm_np] */
  double const *atm_k;          /* [nw][atm_np] */
  double const *atm_pslope;     /* [atm_np] ln-pressure slope to the next level, NaN if not defined */
} jur_view_t;

/* Profile table of a satellite track (ctl->ip == 2, the rule in jurassic_hip.h), rebuilt with every atmosphere by
 * jur_track_profiles and handed to the ray tracer BESIDE the view, as an argument of jur_track_trace_kernel alone: a
 * view that grew would move the later arguments of every kernel and with them every kernel's text.  A profile is a
 * run of points with equal time stamp, longitude and latitude; the profiles of a time block are consecutive. */
typedef struct {
  int ip;                       /* ctl->ip: 1 one profile per time block, 2 the nearest two profiles of the block's track,
                                   3 the weighted mean over the block's cloud (the table of that: jur_cloud_t) */
  int nprof;                    /* profiles of the atmosphere on the device (ip == 2), else 0    */
  double const *x1;             /* [nprof][3] geo2cart(0, lon, lat) of every profile (host libm) */
  double const *lat;            /* [nprof] its latitude                                          */
  int const *first, *len;       /* [nprof] its first atmosphere point and its length (>= 2)      */
  int const *dir;               /* [nprof] its altitude axis: 1 strictly ascending, -1 strictly descending, 0 neither */
  int const *prof_of;           /* [atm_np] profile of every atmosphere point                    */
} jur_track_t;

/* Point cloud (ctl->ip == 3, the rule in jurassic_hip.h): the cached position of every atmosphere point, rebuilt with
 * every atmosphere by jur_cloud_rows, and the influence region.  An argument of jur_cloud_trace_kernel alone, beside
 * the view and NOT inside jur_track_t: either struct, grown, would move the arguments of kernels that exist. */
typedef struct {
  int np;                       /* points the table holds (== view.atm_np while an atmosphere is set), else 0 */
  double cx, cz;                /* ctl->cx, ctl->cz: horizontal and vertical influence length [km], both > 0  */
  double const *x1;             /* [np][3] geo2cart(0, lon, lat) of every atmosphere point (host libm)         */
} jur_cloud_t;

/* One chunk of rays handed to the kernels; all pointers are device memory.
 * Slot i of the chunk works on ray order[i] of the caller's arrays (order ==
 * NULL: ray first+i), so that the caller-visible arrays are indexed by ray id
 * while the workspace arrays (np, tsurf, los) are indexed by slot. */
typedef struct {
  int n;                        /* rays in this chunk                           */
  int stride;                   /* Rt: slots the LOS workspace holds (multiple of 64)           */
  int stride_eps;               /* R: slots the transmittance workspace holds (multiple of 64)  */
  long first;                   /* first ray id when order == NULL              */
  int const *order;             /* [n] ray ids of this chunk, or NULL           */
  double const *geom[7];        /* time, obsz, obslon, obslat, vpz, vplon, vplat; [nr] */
  double *tp[3];                /* tpz, tplon, tplat; [nr]                      */
  double *rad, *tau;            /* [nr][nd]                                     */
  int *np_out;                  /* [nr] LOS points per ray, or NULL             */
  int *np;                      /* [n] LOS points per slot                      */
  double *tsurf;                /* [n]                                          */
  double *los;                  /* tiles of 64 slots: [slot / 64][JUR_NLOS][nfield][64]  */
  double *eps;                  /* path transmittances, tiles of 64 slots: [slot / 64][JUR_NLOS][nd*ng][64] */
  int const *eps_off;           /* [tiles of the chunk] first point slot of every tile in eps when the tiles are laid out
                                   by their longest path instead of JUR_NLOS points each; NULL: tile * JUR_NLOS       */
  int *status;                  /* device flag: bit0 = NLOS overflow            */
  int slice_sorted;             /* neighbouring slots use the same atmosphere slice (one slice, or `order` groups the
                                   rays by slice): the ray tracer may keep a workgroup's slice in LDS            */
  int const *blk_order;         /* [(n + 255) / 256] blocks of 256 slots in the order the launch starts them, longest
                                   paths first (jurk_block_order), or NULL: in order.  Placement only              */
} jur_chunk_t;

/* kernel launchers (jur_kernels.hip); return hipError_t as int */
int jurk_prepare_atm(jur_view_t const *v, double *d_pslope, void *stream);   /* fills atm_pslope */
/* trk->ip == 2: jur_track_trace_kernel (one lane per ray, two profiles per point); trk->ip == 3: jur_cloud_trace_kernel
 * on the table `cld` (one lane per ray, the mean over the block's cloud); else the 1-D tracers by launch */
int jurk_launch_trace(jur_view_t const *v, jur_track_t const *trk, jur_cloud_t const *cld, jur_chunk_t const *c, void *stream);
/* the look-up kernel of the model's band model: cga == 0 emissivity growth (FORMOD 2), != 0 Curtis-Godson (FORMOD 1) */
int jurk_launch_ega(jur_view_t const *v, jur_chunk_t const *c, int cga, void *stream);
int jurk_launch_combine(jur_view_t const *v, jur_chunk_t const *c, void *stream);
/* contributions of the emitters from the transmittance plane of the chunk (after jurk_launch_ega, before the plane is
 * reused; reads c->rad as the NaN mask, so before jurk_launch_combine): rad_c / tau_c [ng + 1][nr][nd] by ray id */
int jurk_launch_contrib(jur_view_t const *v, jur_chunk_t const *c, long nr, double *rad_c, double *tau_c, void *stream);
int jurk_tile_max(int n, int const *d_np, int *d_tile_np, void *stream);
/* dense difference quotients kq[nq][n] from rad[(n + 1) * nq] (nq = rays x channels of the unperturbed block) and steps h[n] */
int jurk_launch_kquot(long nq, long n, double const *d_rad, double const *d_h, double *d_kq, void *stream);   /* longest path per tile of 64 slots */
void jurk_tune_combine(int group, int sync, long min_lanes);
void jurk_tune_trace(int lanes);
void jurk_tune_trace_slice(int mode);
/* Curtis-Godson columns of the traced chunk: outputs [ray][gas][JUR_NLOS], indexed by ray id */
int jurk_launch_cg(jur_view_t const *v, jur_chunk_t const *c, double *cgp, double *cgt, double *cgu, void *stream);
/* bracket records of all n table entries (the last entry of a curve gets slopes nobody reads) */
int jurk_fill_records(jur_ue_t const *ue, jur_rec_t *rec, long long n, void *stream);   /* ue: n + 1 entries */
/* order rays by their geometric tangent altitude: fills order[nr]; `tmp` is a
 * device scratch of jurk_sort_tmp_bytes(nr) bytes */
long jurk_sort_tmp_bytes(long nr);
int jurk_sort_rays(jur_view_t const *v, int by_profile, long nr, double const *d_geom, long ld, int *d_order, void *tmp,
                   long tmp_bytes, void *stream);   /* field k of ray r at d_geom[k * ld + r] */
/* after jurk_sort_rays on the same `tmp`: fills blk_order[(nr + 255) / 256] with the blocks of 256 consecutive slots
 * in ascending order of their lowest ray's tangent altitude (a permutation, whatever the keys) */
int jurk_block_order(long nr, int *d_blk_order, void *tmp, long tmp_bytes, void *stream);

/* the whole path of small calls in one kernel, RB rays per workgroup (c->order is ignored: nothing is sorted) */
long jurk_pencil_lds_bytes(jur_view_t const *v, int RB);
int jurk_launch_pencil(jur_view_t const *v, jur_chunk_t const *c, int RB, void *stream);

/* field-of-view convolution of device arrays: rad0/tau0 [nr][nd] -> rad/tau [nr][ld]; status bit 1: a ray alone in its scan */
int jurk_launch_fov(long nr, int nd, double const *time, double const *vpz, double const *rad0, double const *tau0, double *rad,
                    double *tau, long ld, int n, double const *dz, double const *w, int *status, void *stream);

/* atmosphere regridding (intpol_atm): device rows as documented at jur_intpol_kernel */
int jurk_launch_intpol(int ip, int ng, int nw, int ns, int nd_, int nx, double cx, double cz, double const *src, double const *x1,
                       int const *idx, int const *nz, double const *dst, double const *x0, double *out, void *stream);

/* known-answer hooks (tests): device functions on arrays, see jurassic_hip.h */
int jurk_kat_ega(jur_view_t const *v, int g, int d, long n, double const *tau, double const *t, double const *u, double const *p,
                 int mode, int chain, double *out, void *stream);
int jurk_kat_cga(jur_view_t const *v, int g, int d, long n, double const *tau, double const *cgt, double const *cgu, double const *cgp,
                 int mode, int chain, double *out, void *stream);
int jurk_kat_continua(jur_view_t const *v, int d, long n, double const *p, double const *t, double const *q, double const *u_co2,
                      double const *u_h2o, double *out, void *stream);
int jurk_kat_update(jur_view_t const *v, int d, long n, int what, double const *a, double const *b, double const *c, double *rad,
                    double *tau, double *src, void *stream);
/* rule 4 of IP 3 at n positions given after the geometry step: z0, lat0 [n], x0 [n][3] -> out [2 + ng + nw][n] */
int jurk_kat_cloud_mean(jur_view_t const *v, jur_cloud_t const *cld, long n, int a0, int len, double const *z0, double const *lat0,
                        double const *x0, double *out, void *stream);
int jurk_cloud_lds_points(void);
/* LOS records of the traced chunk (after jurk_launch_trace): los[ray][nfield][JUR_NLOS], tsurf[ray], indexed by ray id */
int jurk_kat_los(jur_view_t const *v, jur_chunk_t const *c, double *los, double *tsurf, void *stream);

/* Block Jacobian of a scene (jur_kernel_scene_host).  The stacked atmosphere is a list of copies: copy 0 is the base
 * atmosphere, copy j >= 1 the points of one slice with one state element raised.  All arrays are device memory. */
typedef struct {
  int ncopy;                    /* copies, the base included                                              */
  int np0;                      /* points of the base atmosphere (row length of `base`)                   */
  int nrow;                     /* rows of an atmosphere: 6 + ng + nw                                      */
  int ng;
  long nt;                      /* points of the stacked atmosphere (row length of `rows`)                */
  long const *off;              /* [ncopy + 1] first stacked point of every copy; off[ncopy] = nt         */
  int const *first;             /* [ncopy] first base point of the copy                                    */
  int const *prow;              /* [ncopy] row of the raised value (-1: the base)                          */
  int const *pip;               /* [ncopy] base point of the raised value                                  */
  double const *base;           /* [nrow][np0] base rows (time stamps as stack_times leaves them)          */
  double *rows;                 /* [nrow][nt] stacked rows, written                                        */
  double *h;                    /* [ncopy] step of every copy, written (h[0] is not)                       */
  double tmax, span;            /* copy j >= 1 carries the time stamp tmax + j * span                      */
} jur_scene_stack_t;

/* one pass: the rays [r0, r1) of the call, ray r replicated width[r] + 1 times from slot off(r) =
 * (rowptr[r] - rowptr[r0]) + (r - r0) of the pass on */
typedef struct {
  long nr;                      /* rays of the call (row length of in_geom, out_tp)                        */
  long r0, r1;
  int nd;
  long const *rowptr;           /* [nr + 1]                                                                */
  int const *first, *len;       /* [nr] slice of every ray in the base atmosphere                          */
  int const *copy0;             /* [nr] copy that raises the first state element of the ray's slice        */
  long const *off;              /* [ncopy + 1] as jur_scene_stack_t                                        */
  double const *atm_time;       /* [nt] time stamps of the stacked atmosphere                              */
  double above;                 /* a time stamp above all of them                                          */
  double const *in_geom;        /* [7][nr] the caller's geometry                                           */
  double const *in_rad;         /* [nr][nd] the caller's radiances (NaN mask)                              */
  long n;                       /* slots of the pass                                                       */
  double *geom;                 /* [7][n] replicated geometry, written                                     */
  double *rad, *tau, *tp;       /* [n][nd], [n][nd], [3][n] of the pass: rad written (mask), then the forward model's */
  int *np;                      /* [n]                                                                     */
  double const *h;              /* [ncopy]                                                                 */
  double *k;                    /* [(rowptr[r1] - rowptr[r0]) * nd] blocks of the pass, written            */
  double *out_rad, *out_tau;    /* [nr][nd] unperturbed results by ray, written                            */
  double *out_tp;               /* [3][nr]                                                                 */
  int *out_np;                  /* [nr]                                                                    */
  double const *fov_tau;        /* [r1 - r0][nd] convolved transmittances of copy 0 by ray of the pass (a field of view is
                                   set: jurk_scene_fov), or NULL: out_tau is gathered from tau                */
} jur_scene_pass_t;

int jurk_scene_stack(jur_scene_stack_t const *a, void *stream);
int jurk_scene_rays(jur_scene_pass_t const *a, void *stream);      /* geometry and mask of the pass */
int jurk_scene_quot(jur_scene_pass_t const *a, long nk, void *stream);   /* the nk block elements and the unperturbed results of the pass */

/* Normal equations of a scene (jur_normal_scene_host): per distinct slice s of width w_s the sums over its live
 * measurements, kept in device memory across the passes.  One workgroup per 16 x 16 tile of the lower triangle of A_s. */
typedef struct {
  long nslice;
  long const *tptr;             /* [nslice + 1] running sum of the tiles T (T + 1) / 2, T = ceil(w_s / 16)  */
  long const *sptr;             /* [nslice + 1] rays of every slice in srays                                */
  int const *srays;             /* the rays of every slice, ascending                                       */
  long const *wptr, *aptr;      /* [nslice + 1] running sums of w_s and of w_s^2                             */
  double const *y, *weight;     /* [nr][nd] measurements and the diagonal of their inverse covariance       */
  double *A, *b, *cost;         /* [aptr[nslice]], [wptr[nslice]], [nslice] accumulators, read and written   */
  long *nlive;                  /* [nslice]                                                                 */
} jur_scene_normal_t;
/* the terms of the rays [a->r0, a->r1) from the blocks a->k and the results a->out_rad of the pass (after jurk_scene_quot) */
int jurk_scene_normal(jur_scene_pass_t const *a, jur_scene_normal_t const *n, long ntiles, void *stream);

/* Gradient of a scene from blocks that are held (jur_gradient_scene_host, the reuse iterations of jur_retrieve_scene_host):
 * b, cost and nlive of jur_scene_normal_t alone, from the results a->out_rad of a forward-only pass (after
 * jurk_scene_quot) and the block of ray r of the call at k + koff[r], [nd][w].  gptr cuts every slice into workgroups of
 * 256 state elements. */
typedef struct {
  double const *k;              /* the blocks, wherever the Jacobian pass or the caller left them           */
  long const *koff;             /* [nr] first double of the block of every ray of the call                  */
  long const *gptr;             /* [nslice + 1] running sum of ceil(w_s / 256)                              */
} jur_scene_grad_t;
int jurk_scene_gradient(jur_scene_pass_t const *a, jur_scene_normal_t const *n, jur_scene_grad_t const *g, long ngroups, void *stream);

/* Levenberg-Marquardt step of a scene (jur_solve_slices_host, jur_step_scene_host): the damped, optionally regularised
 * system of every slice under one damping each, one workgroup per system.  All arrays are device memory. */
typedef struct {
  long nslice;
  long const *wptr, *aptr;      /* [nslice + 1] running sums of w_s and of w_s^2                             */
  double const *A, *b;          /* [aptr[nslice]], [wptr[nslice]] read only: diagonal and lower triangle of A_s */
  double const *lam;            /* [nslice] the damping of every system                                     */
  double const *prior_ivar, *prior_dx;   /* [wptr[nslice]] each, or both NULL                                */
  int mode;                     /* JUR_DAMP_MARQUARDT or JUR_DAMP_PRIOR                                      */
  double *M;                    /* [aptr[nslice]] scratch: M_s, factored in place; L_s afterwards             */
  double *live;                 /* [wptr[nslice]] scratch: D_i of a live element, 0 of a dead one             */
  double *dx;                   /* [wptr[nslice]] g, then z, then the step, written                           */
  double *pred;                 /* [nslice] written                                                         */
  int *status;                  /* [nslice] written: 0, or 1 + the column whose pivot was not > 0            */
  int const *state;             /* [nslice] or NULL: a system whose state is not 0 is left alone (jur_retrieve_scene_host) */
} jur_scene_solve_t;
int jurk_scene_solve(jur_scene_solve_t const *a, void *stream);

/* Posterior diagnostics of a scene (jur_diagnose_slices_host, jur_diagnose_scene_host), after jurk_scene_solve with
 * lam = 0 and a zero right-hand side has left L_s in `L`, D_i in `live` and the breakdowns in `status`.  All arrays are
 * device memory.  S and avk are always formed: what the caller did not ask for stays on the device. */
typedef struct {
  long nslice;
  long const *wptr, *aptr;      /* [nslice + 1] running sums of w_s and of w_s^2                             */
  double const *A;              /* [aptr[nslice]] read only: diagonal and lower triangle of A_s              */
  double const *prior_ivar;     /* [wptr[nslice]] or NULL                                                   */
  double const *L;              /* [aptr[nslice]] the factors                                               */
  double const *live;           /* [wptr[nslice]] D_i of a live element, 0 of a dead one                     */
  int const *status;            /* [nslice] 0, or 1 + the column of the breakdown                            */
  int const *imap;              /* [ninv][2] column block -> (system, first column), 16 columns a block       */
  int const *tmap;              /* [ntile][3] output tile -> (system, first row, first column), 64 x 64       */
  double *S, *avk;              /* [aptr[nslice]] each, written                                             */
  double *sigma, *sigma_noise, *sigma_smooth, *avk_diag;   /* [wptr[nslice]] each, written                   */
  double *dofs;                 /* [nslice] written                                                         */
} jur_scene_diag_t;
/* S, then AVK, then the vectors: four launches in stream order (nb = wptr[nslice]; the block counts are the host's) */
int jurk_scene_diag(jur_scene_diag_t const *a, long ninv, long ntile, long nb, void *stream);
enum { JUR_DIAG_NB = 16, JUR_DIAG_TILE = 64 };
/* host arithmetic of the diagnostics (jur_scene.c; no GPU): the refusals, and the two block maps of jur_scene_diag_t
 * (either may be NULL: a first call counts).  jur_diag_maps returns the number of column blocks and sets *ntile. */
int jur_diag_check_out(char const *who, jur_diag_out_t const *out);
int jur_diag_check_wptr(char const *who, long nslice, long const *wptr);
int jur_diag_check_prior(char const *who, long nslice, long const *wptr, double const *prior_ivar);
long jur_diag_maps(long nslice, long const *wptr, int *imap, int *tmap, long *ntile);
/* Gain matrix and error budget of a scene (jur_gain_slices_host, jur_gain_scene_host), after the diagnostics have left
 * S_s and the breakdowns on the device.  Measurement m of slice s is channel m % nd of ray srays[sptr[s] + m / nd]; its
 * block row lies at k + koff[ray] + channel * w_s and its gain row at the same place in `gain`.  All arrays are device
 * memory. */
typedef struct {
  long nslice;
  int nd, ncomp;
  long const *wptr, *aptr;      /* [nslice + 1] running sums of w_s and of w_s^2                             */
  long const *sptr;             /* [nslice + 1] rays of every slice in srays                                */
  int const *srays;             /* the rays of every slice, ascending                                       */
  long const *koff;             /* [nr] first double of the block of every ray of the call                  */
  long const *gptr;             /* [nslice + 1] running sum of ceil(w_s / 256): the budget's workgroups      */
  int const *gmap;              /* [ntile][3] gain tile -> (slice, first measurement, first element), 64 x 64 */
  int const *status;            /* [nslice] or NULL: a system whose status is not 0 is all +0.0              */
  double const *S;              /* [aptr[nslice]] posterior covariances                                     */
  double const *k;              /* the blocks                                                               */
  double const *weff;           /* [nr][nd] effective weights: anything not > 0 is "not live"                */
  double const *var;            /* [ncomp][nrd] variances per component                                     */
  long nrd, nb;                 /* nr * nd; wptr[nslice]                                                     */
  double *gain;                 /* laid out as k, written                                                   */
  double *sigc;                 /* [ncomp][nb] written                                                      */
} jur_scene_gain_t;
/* the gain, then (ncomp > 0) the budget, in stream order */
int jurk_scene_gain(jur_scene_gain_t const *a, long ntile, long ngroups, void *stream);
/* weff = weight where mask, f and y are finite and weight > 0, else 0; n values each */
typedef struct { long n; double const *mask, *f, *y, *weight; double *weff; } jur_scene_weff_t;
int jurk_scene_weff(jur_scene_weff_t const *a, void *stream);
enum { JUR_GAIN_TILE = 64, JUR_GAIN_MAXCOMP = 8 };
/* host arithmetic of the gain entries (jur_scene.c; no GPU): the refusals and the tile map.  jur_gain_check_layout: sid in
 * -1 .. nslice - 1 and the width of every ray that of its slice (0 without one).  jur_gain_check_var: every variance of a
 * measurement with live[r * nd + id] != 0 is >= 0 and finite.  jur_gain_maps: tile t of the product is the measurements
 * [m0, m0 + 64) x the elements [i0, i0 + 64) of slice s, gmap[3 t] = s, then m0, i0, slices ascending, row-major within
 * a slice; gmap may be NULL (a first call counts); returns the number of tiles, -1 for a slice with 2^31 measurements. */
int jur_gain_check_args(char const *who, jur_gain_in_t const *in, jur_gain_out_t const *out);
int jur_gain_check_layout(char const *who, long nslice, long const *wptr, long nr, long const *rowptr, int const *sid);
int jur_gain_check_var(char const *who, int ncomp, long nr, int nd, double const *var, unsigned char const *live);
long jur_gain_maps(long nslice, long const *wptr, long const *sptr, int nd, int *gmap);
/* Parameter errors of a scene (jur_param_slices_host): C_s = G_s^T Kb_s over the live measurements of every slice, then
 * the quadratic forms on it.  Measurements and the rows of `gain` as in jur_scene_gain_t; the row of kb of the same
 * measurement lies at kb + koffb[ray] + channel * wb_s.  All arrays are device memory. */
typedef struct {
  long nslice;
  int nd, nvar, ncov;
  long const *wptr, *bwptr;     /* [nslice + 1] running sums of w_s and of wb_s                              */
  long const *cptr, *bbptr;     /* [nslice + 1] running sums of w_s * wb_s and of wb_s^2                     */
  long const *sptr;             /* [nslice + 1] rays of every slice in srays                                */
  long const *pptr;             /* [nslice + 1] running sum of ceil(w_s / 64): the quadratic forms' workgroups */
  int const *srays;             /* the rays of every slice, ascending                                       */
  long const *koff, *koffb;     /* [nr] first double of the gain block and of the kb block of every ray     */
  int const *cmap;              /* [ntile][3] tile of C -> (slice, first i, first j), 64 x 64                */
  double const *gain, *kb;      /* the blocks                                                               */
  double const *weff;           /* [nr][nd] effective weights: anything not > 0 is "not live"                */
  double const *var;            /* [nvar][nbw] diagonal parameter covariances                               */
  double const *cov;            /* [ncov][nbb] full ones                                                    */
  long nb, nbw, nbb;            /* wptr[nslice], bwptr[nslice], bbptr[nslice]                                */
  double *C;                    /* [cptr[nslice]] written                                                   */
  double *sig;                  /* [nvar + ncov][nb] written                                                */
} jur_scene_param_t;
/* the cross-state matrices, then (nvar + ncov > 0) the quadratic forms, in stream order */
int jurk_scene_param(jur_scene_param_t const *a, long ntile, long ngroups, void *stream);
/* jur_param_scene_host: the chains of C continued over the rays of one pass, C read and written in place.  pmap: [ntile][5]
 * as jur_param_pass_maps makes it; the kb row of a ray lies in a->kb at koffb[ray] - kb0 (the buffer of the pass); of *a
 * cmap, pptr, var, cov and sig are not read. */
int jurk_scene_cross_pass(jur_scene_param_t const *a, int const *pmap, long ntile, long kb0, void *stream);
enum { JUR_PARAM_TILE = 64, JUR_PARAM_ROWS = 64, JUR_PARAM_MAXCOMP = 8 };
/* host arithmetic of jur_param_slices_host (jur_scene.c; no GPU).  jur_param_layout_as: jur_param_layout under the name
 * `who` in its messages.  jur_param_check_args: the structs.  jur_param_check_bwptr: bwptr against the widths of the rays.
 * jur_param_check_values: var >= 0 and finite; what is read of cov finite, its diagonal >= 0.  jur_param_maps: tile t of C
 * is the elements [i0, i0 + 64) x the parameters [j0, j0 + 64) of slice s, cmap[3 t] = s, then i0, j0, slices ascending,
 * row-major within a slice; cmap may be NULL (a first call counts); returns the number of tiles. */
long jur_param_layout_as(char const *who, long nslice, long const *wptr, long nr, long const *rowptr, long const *rowptr_b,
                         int const *sid, long *bwptr, long *cptr, long *bbptr);
int jur_param_check_args(char const *who, jur_param_in_t const *in, jur_param_out_t const *out);
int jur_param_check_bwptr(char const *who, long nslice, long const *bwptr, long const *bw);
int jur_param_check_values(char const *who, long nslice, long const *bwptr, long const *bbptr, jur_param_in_t const *in);
long jur_param_maps(long nslice, long const *wptr, long const *bwptr, int *cmap);
/* the passes of jur_param_scene_host (jur_scene.c; no GPU).  jur_param_pass_range: the stretch [*lo, *hi) of srays (the
 * ascending ray list of slice s at sptr[s] .. sptr[s + 1]) that holds its rays inside [r0, r1); empty: *lo == *hi.
 * jur_param_pass_maps: the tiles of C of the slices that have rays in [r0, r1), in the order the rays of the pass first
 * meet them, row-major within a slice: pmap[5 t] = s, then i0, j0 as jur_param_maps, then lo, hi of jur_param_pass_range.
 * mark [nslice] is the caller's scratch, all zeros before the first pass of a call and carried from pass to pass (passes
 * are told apart by r0: each is mapped once); pmap has room for the tiles of all slices, jur_param_maps' count.  Returns
 * the number of tiles. */
void jur_param_pass_range(long const *sptr, int const *srays, long s, long r0, long r1, long *lo, long *hi);
long jur_param_pass_maps(long const *wptr, long const *bwptr, long const *sptr, int const *srays, int const *sid, long r0, long r1,
                         long *mark, int *pmap);
/* host checks of the full prior precision (jur_scene.c; no GPU): what is read of R, the layout of a call against the one
 * set, the arguments of jur_prior_corr_host */
int jur_prior_check_R(char const *who, long nslice, long const *wptr, double const *R);
int jur_prior_check_layout(char const *who, long set_nslice, long const *set_wptr, long nslice, long const *wptr);
int jur_prior_check_corr(char const *who, long nslice, long const *wptr, int const *iq, double const *z, double const *sigma,
                         int nq, double const *cz);

/* Trial states of a scene (jur_trial_scene_host, jur_retrieve_scene_host): the state elements of the slices where they
 * lie in the base rows, and ntrial candidate steps of each.  The trial atmosphere is stacked like the Jacobian's: copy 0
 * the base, copy 1 + s * ntrial + t the points of slice s with all its elements moved by dx[t].  All arrays are device
 * memory. */
typedef struct {
  long nslice;
  int ntrial, np0;
  long nt;                      /* points of the stacked trial atmosphere (row length of `rows`)            */
  long const *wptr;             /* [nslice + 1] running sum of the widths                                   */
  long const *off;              /* [1 + nslice * ntrial + 1] first stacked point of every copy              */
  int const *sfirst;            /* [nslice] first base point of every slice                                 */
  int const *erow, *eip;        /* [wptr[nslice]] row and base point of every state element                 */
  int const *state;             /* [nslice] or NULL: slices whose state is not 0 take no part               */
  int const *choice;            /* [nslice] JUR_ELEM_ACCEPT: the accepted trial, -1 for none                */
  double *base;                 /* [nrow][np0] base rows; written by JUR_ELEM_ACCEPT only                   */
  double const *dx;             /* [ntrial][wptr[nslice]]                                                   */
  double *rows;                 /* [nrow][nt] stacked rows (after jurk_scene_stack); the moved values are written */
  double const *ivar, *xa;      /* [wptr[nslice]] diagonal prior (jurk_scene_prior, JUR_ELEM_PRIOR_DX)      */
  double *prior;                /* [ntrial][nslice] written by jurk_scene_prior ([nslice] with dx == NULL)  */
  double *out;                  /* [wptr[nslice]] written by JUR_ELEM_PRIOR_DX (xa - x) and JUR_ELEM_STATE (x) */
  double const *lo, *hi;        /* [wptr[nslice]] the box of every element (jur_model_set_state_bounds), or both NULL:
                                 * where x + dx is formed, JUR_STATE_BOUND of it takes its place                    */
} jur_scene_trial_t;
/* the rule of jur_state_bound, one text for host and device: a NaN x gives lo, an infinite bound does not bind */
#define JUR_STATE_BOUND(c, x, lo, hi) do { (c) = (x) > (lo) ? (x) : (lo); (c) = (c) < (hi) ? (c) : (hi); } while (0)
enum { JUR_ELEM_APPLY = 0, JUR_ELEM_PRIOR_DX = 1, JUR_ELEM_ACCEPT = 2, JUR_ELEM_STATE = 3 };
/* one lane per state element (JUR_ELEM_APPLY: per trial and element) of the nb = wptr[nslice]: what `op` says */
int jurk_scene_elements(jur_scene_trial_t const *a, int op, long nb, void *stream);
/* prior[t][s] = sum_i r_i (xa_i - (x_i + dx[t][i]))^2 as a chain of separately rounded operations, ascending i; with
 * dx == NULL the one row of the state as it stands */
int jurk_scene_prior(jur_scene_trial_t const *a, void *stream);

/* one pass of trial rays: the rays [r0, r1) of the call, each replicated ntrial times, slot (r - r0) * ntrial + t */
typedef struct {
  long nr, r0, r1;
  int nd, ntrial;
  int const *first, *len;       /* [nr] slice of every ray in the base atmosphere                          */
  int const *tcopy0;            /* [nr] trial copy 0 of the ray's slice, 0 for a ray without state elements */
  long const *off;              /* as jur_scene_trial_t                                                    */
  double const *atm_time;       /* [nt] time stamps of the stacked trial atmosphere                        */
  double above;
  double const *in_geom;        /* [7][nr]                                                                 */
  double const *in_rad;         /* [nr][nd] NaN mask                                                       */
  long n;                       /* slots of the pass                                                       */
  double *geom, *rad;           /* [7][n], [n][nd] of the pass: written, rad then by the forward model     */
  long nslice;
  long const *sptr;             /* [nslice + 1] as jur_scene_normal_t                                      */
  int const *srays;
  int const *state;             /* [nslice] or NULL                                                        */
  double const *y, *weight;     /* [nr][nd]                                                                */
  double *cost;                 /* [ntrial][nslice] accumulators, read and written                         */
} jur_scene_trial_pass_t;
int jurk_scene_trial_rays(jur_scene_trial_pass_t const *a, void *stream);   /* geometry and mask of the pass */
int jurk_scene_trial_cost(jur_scene_trial_pass_t const *a, void *stream);   /* after the forward model on the pass */

/* the rays act[0 .. n) of a call gathered into arrays of their own (jur_retrieve_scene_host: the rays of the slices
 * that are still active) */
typedef struct {
  long nr, n;                   /* rays of the call, rays gathered                                          */
  int nd;
  int const *act;               /* [n] ascending                                                            */
  double const *geom, *rad, *y, *weight;   /* [7][nr], [nr][nd] x 3                                          */
  int const *first, *len, *copy0, *tcopy0; /* [nr]                                                          */
  double *geom_c, *rad_c, *y_c, *weight_c; /* [7][n], [n][nd] x 3                                            */
  int *first_c, *len_c, *copy0_c, *tcopy0_c;   /* [n]                                                        */
  double const *live;           /* [nr][nd] effective mask of a field of view, or NULL                      */
  double *live_c;               /* [n][nd]                                                                  */
} jur_scene_compact_t;
int jurk_scene_compact(jur_scene_compact_t const *a, void *stream);

/* Untraceable rays of a pass (jur_model_set_scene_overflow): the rule of jur_np_overflows, one text for host and device --
 * the tracer clamps a ray that needs JUR_NLOS points or more to JUR_NLOS - 1 and keeps no flag of its own, so a ray that
 * fills the array counts, clamped or not */
#define JUR_NP_OVERFLOWS(np) ((np) >= JUR_NLOS - 1)
#define JUR_OVERFLOW_PARTS 256  /* the most workgroups of the fold kernel: one partial count each */
/* one lane per slot of a pass, after its forward model: flag[t][s] = 1 where slot (ray r of slice s, trial t) holds such a
 * ray.  A trial pass has ntrial slots per ray, slot (r - r0) * ntrial + t; a Jacobian or forward-only pass (ntrial == 0)
 * has the slots of rowptr (width + 1 per ray, one with the all-zero rowptr) and one row of flags.  The slice of ray r is
 * (tcopy0[r] - 1) / per, tcopy0 as jur_scene_trial_pass_t's; a ray without state elements (tcopy0 == 0) sets nothing. */
typedef struct {
  long n, r0, r1;               /* slots of the pass, its rays                                              */
  int ntrial, per;
  long nslice;
  long const *rowptr;           /* ntrial == 0: as jur_scene_pass_t                                         */
  int const *tcopy0;            /* [nr]                                                                     */
  int const *np;                /* [n] LOS points of every slot (the forward model's)                       */
  int *flag;                    /* [max(ntrial, 1)][nslice]; written with 1 only, zeroed by the caller      */
} jur_scene_ovf_t;
int jurk_scene_overflow(jur_scene_ovf_t const *a, void *stream);
/* the fold, one lane per flag (at most JUR_OVERFLOW_PARTS workgroups, each striding over the flags): with cost given,
 * cost[t][s] = NaN where flag[t][s] and slice s takes part (state NULL or state[s] == 0); without, state[s] =
 * JUR_RET_FAILED where flag[s] and state[s] == 0.  part[g] is the number of cells workgroup g changed. */
typedef struct {
  long nslice;
  int ntrial;
  int const *flag;
  int *state;                   /* [nslice]; written only without cost                                      */
  double *cost;                 /* [ntrial][nslice] or NULL                                                 */
  long *part;                   /* [jur_scene_overflow_parts(lanes)]                                        */
} jur_scene_ovfold_t;
int jurk_scene_overflow_fold(jur_scene_ovfold_t const *a, void *stream);
long jur_scene_overflow_parts(long lanes);   /* workgroups of the fold over that many flags (jur_scene.c) */

/* Full a-priori precision of the slices (jur_model_set_prior_precision): P_s = R_s + diag(r_s), R_s [w][w] of which the
 * diagonal and the lower triangle are read, r = prior_ivar.  The existing kernels run unchanged on what these form.  All
 * arrays are device memory; wptr, aptr lay out the systems as jur_scene_solve_t's. */
typedef struct {
  long nslice;
  long const *wptr, *aptr;
  double const *A;              /* [aptr[nslice]] diagonal and lower triangle read; NULL: P alone, nothing masked  */
  double const *b;              /* [wptr[nslice]], or NULL: g is not formed                                         */
  double const *R;              /* [aptr[nslice]]                                                                   */
  double const *ivar, *d;       /* [wptr[nslice]] r and prior_dx (d is read with b only)                            */
  double const *lam;            /* [nslice] JUR_DAMP_PRIOR: M = A + P + lam P; NULL: M = A + P                      */
  double *M;                    /* [aptr[nslice]] written: diagonal and lower triangle; 0 in a dead row or column   */
  double *g;                    /* [wptr[nslice]] written with b: fma(r_i, d_i, b_i) + (R d)_i over live j, 0 if dead */
  int const *state;             /* [nslice] or NULL: a system whose state is not 0 is left alone                    */
} jur_scene_pasm_t;
/* one wavefront per row (nb = wptr[nslice] rows) */
int jurk_scene_prior_assemble(jur_scene_pasm_t const *a, long nb, void *stream);

/* quadratic forms v^T R v of nvec vectors per system, and what is made of them */
typedef struct {
  long nslice;
  int nvec;
  long const *wptr, *aptr;
  double const *R;              /* [aptr[nslice]]                                                                   */
  double const *v;              /* [nvec][wptr[nslice]]                                                             */
  double *out;                  /* [nvec][nslice] read and written: out += v^T R v                                  */
  int const *state;             /* [nslice] or NULL                                                                 */
  /* jurk_scene_prior_pred (nvec == 1, v the step): out = sum_i v_i fma(lam r_i, v_i, g_i) over the live elements in the
   * solve kernel's order, + lam v^T R v; a system with status != 0 keeps its 0 */
  double const *lam, *ivar, *g, *live;
  int const *status;
} jur_scene_pquad_t;
int jurk_scene_prior_quad(jur_scene_pquad_t const *a, void *stream);
int jurk_scene_prior_pred(jur_scene_pquad_t const *a, void *stream);
/* d[t][e] = xa[e] - (x_e + dx[t][e]) (dx == NULL: the one row xa - x) into a->out, one lane per trial and element */
int jurk_scene_prior_diff(jur_scene_trial_t const *a, long nb, void *stream);
/* sigma_smooth_i = sqrt(max(sum_j (S P)_ij S_ij, 0)): the product by jur_scene_avk_kernel with P (a->A) in A's place
 * into a->avk, then one wavefront per row; a->sigma_smooth alone is written */
int jurk_scene_prior_smooth(jur_scene_diag_t const *a, long ntile, long nb, void *stream);
/* jur_scene_inverse_kernel alone: S from the factor (jur_prior_corr_host) */
int jurk_scene_prior_inverse(jur_scene_diag_t const *a, long ninv, void *stream);
/* Sa of jur_prior_corr_host: one lane per entry of the lower triangles, mirrored */
typedef struct {
  long nslice;
  long const *wptr, *aptr;
  int const *iq;                /* [wptr[nslice]] quantity of every element                                         */
  double const *z, *sigma;      /* [wptr[nslice]]                                                                   */
  int nq;
  double const *cz;             /* [nq]                                                                             */
  double *Sa;                   /* [aptr[nslice]] written, full                                                     */
} jur_scene_pcov_t;
int jurk_scene_prior_cov(jur_scene_pcov_t const *a, long na, void *stream);

/* Field of view of the scene entries (jur_model_set_fov): the forward model's results of one pass, replicated as the
 * pass lays them out, convolved out of place with the shape of the model.  Ray r of [r0, r1) owns `count` consecutive
 * slots from `slot`, nd values each: with ntrial == 0 (a Jacobian pass) slot = (rowptr[r] - rowptr[r0]) + (r - r0) and
 * count = width + 1, with ntrial >= 1 (a trial pass, or plain rays with ntrial == 1) slot = (r - r0) * ntrial and count =
 * ntrial.  Value v of the ray's count * nd is convolved with value v of the rays of its window: those of [r - JUR_NFOV,
 * r + JUR_NFOV] inside the pass with its time stamp (a scan lies in one pass and its rays have one width). */
typedef struct {
  long nr, r0, r1;
  int nd, ntrial;
  long const *rowptr;           /* [nr + 1] (ntrial == 0)                                                   */
  double const *time, *vpz;     /* [nr] the caller's time stamps and view-point altitudes                   */
  double const *rad;            /* [n][nd] the forward model's                                              */
  double const *tau;            /* [n][nd], or NULL                                                         */
  double *rad_f;                /* [n][nd] written                                                          */
  double *tau_f;                /* [r1 - r0][nd] written where tau is given: the first nd values of every ray */
  int n;                        /* points of the shape                                                      */
  double const *dz, *w;         /* [n]                                                                      */
  int *status;                  /* bit 1: a window of fewer than two rays                                   */
} jur_scene_fov_t;
int jurk_scene_fov(jur_scene_fov_t const *a, void *stream);

/* Hydrostatic balance of the segments of a scene (jur_model_set_scene_hydz): segment i is the points [at[i], at[i] +
 * len[i]) of the rows given -- of the base rows [nrow][np0] or of the stacked rows [nrow][nt].  One wavefront per segment;
 * p alone is written, and p of the segment's reference parcel is not.  All arrays are device memory. */
typedef struct {
  long nseg;
  long const *at;               /* [nseg] first point of every segment within a row                        */
  int const *len;               /* [nseg] points of every segment; fewer than 2: left alone                 */
  double const *z, *lat, *t;    /* rows                                                                    */
  double const *q;              /* the H2O row, or NULL: dry air                                           */
  double *p;                    /* the pressure row, written                                               */
  double hydz;
} jur_scene_hydro_t;
int jurk_scene_hydro(jur_scene_hydro_t const *a, void *stream);

/* host arithmetic shared by jur_model.c and jur_scene.c (not exported) */
#define JUR_HIDDEN __attribute__((visibility("hidden")))
JUR_HIDDEN int jur_atm_slice(double const *time, long n, double t, long *first);
/* jur_track_profiles on rows (jur_track.c), with the altitude direction of every profile and the profile of every point */
JUR_HIDDEN long jur_track_rows(long n, double const *time, double const *z, double const *lon, double const *lat, int *first,
                               int *len, double (*x1)[3], int *block_of, int *dir, int *prof_of);
/* jur_cloud_points on rows (jur_cloud.c) */
JUR_HIDDEN long jur_cloud_rows(long n, double const *lon, double const *lat, double (*x1)[3]);
JUR_HIDDEN size_t jur_state_vector(ctl_t const *ctl, atm_t const *atm, double *x, int *iqa, int *ipa);
JUR_HIDDEN long jur_scene_slice_elements(ctl_t const *ctl, atm_t const *atm, int first, int len, long *cols, int *iqa, int *ipa);
/* a distinct slice of a scene: points [first, first + len) with nel state elements; next: chain of the slices that
 * share the first point */
typedef struct { int first, len, next; long nel; } jur_scene_slice_t;
JUR_HIDDEN long jur_scene_distinct(int np, long nr, int const *first, int const *len, long const *rp, int *sid, jur_scene_slice_t **out);
/* the per-quantity box of jur_model_set_state_bounds laid out per element (jur_scene.c; no GPU): elo[e] = lo[iq], ehi[e] =
 * hi[iq] with iq = erow[e] - 4, the quantity of the row that jur_scene_trial_t's erow names; and the check of a box
 * (JUR_EINVAL naming the quantity: nq is not nq_model, a NaN, lo > hi) */
JUR_HIDDEN void jur_state_bounds_expand(double const *lo, double const *hi, long n, int const *erow, double *elo, double *ehi);
JUR_HIDDEN int jur_state_bounds_check(char const *who, int ng, int nw, int nq, double const *lo, double const *hi);

/* hydrostatic_1d_h2o on one profile of n points (jur_scene.c): what jur_model_set_atm's step and jur_scene_hydrostatic
 * both run; qh2o == NULL: dry air */
JUR_HIDDEN void jur_hydrostatic_profile(double hydz, int n, double const *z, double const *lat, double const *t, double const *qh2o,
                                        double *p);
/* the refusals of a balance's segments (outside 0..np; two segments of two points or more that share a point), and the
 * distinct slices of two points or more among the rays' (first, len) */
JUR_HIDDEN int jur_scene_hydro_check(char const *who, int np, long nseg, int const *sfirst, int const *slen);
JUR_HIDDEN long jur_scene_ray_slices_of(int np, long nr, int const *first, int const *len, int *sfirst, int *slen);
/* segments of the balance as one value: n of them, their first points and lengths (host or device memory) */
typedef struct { long n; long const *at; int const *len; } jur_hyseg_t;
static inline jur_hyseg_t jur_hyseg_sub(jur_hyseg_t h, long from, long n) { jur_hyseg_t const o = {n, h.at + from, h.len + from}; return o; }
/* The segment lists of a scene entry, malloc'ed as at[nh] with the ints len[nh] behind (NULL: out of memory): the nrs ray
 * slices (hyf: first | len, nr apart); of the copies 1 .. ncopy - 1 laid out by off those whose raised row prow[j] the
 * pressures depend on (p, T, row_h2o), *nhc of them; the trial copies 1 .. tncopy - 1 laid out by toff, *ntc of them */
JUR_HIDDEN long *jur_scene_hydro_segments(size_t nh, long nr, long nrs, int const *hyf, long ncopy, long const *off, int const *prow,
                                          int row_h2o, long tncopy, long const *toff, long *nhc, long *ntc);
/* the default cap on the slots of a pass: a sixteenth of what `used` bytes leave of the workspace budget, in slots of
 * slot_bytes; never fewer than 4096, a few hundred KB, so that a small budget does not end in a pass and a wait per ray */
JUR_HIDDEN long jur_scene_default_cap(long budget, long used, size_t slot_bytes);
/* the rays of every slice as one CSR (sid[r] < 0: a ray without state elements, in no list): sptr[nslice + 1], srays[up
 * to nr], the rays of a slice ascending; returns the length of the lists */
JUR_HIDDEN long jur_scene_rays_by_slice(long nr, long nslice, int const *sid, long *sptr, int *srays);
/* the rays of the slices whose state is JUR_RET_ACTIVE, in arrays of their own: act[n] the rays in their order, pos[nr]
 * where each went (-1: it left), rpc[n + 1] their rowptr, sptrc[nslice + 1] | sraysc[sptrc[nslice]] the lists of sptr |
 * srays in the new positions (an ended slice's is empty); returns n */
JUR_HIDDEN long jur_scene_gather_active(long nr, long nslice, long const *rp, int const *sid, int const *state, long const *sptr,
                                        int const *srays, int *act, int *pos, long *rpc, long *sptrc, int *sraysc);

/* internals of a model that jur_multi.c needs (jur_model.c) */
/* jur_formod_device on rays that are part of larger arrays: geometry field k at d_geom + k * ldg, tangent-point field k
 * at d_tp + k * ldtp (jur_formod_device: ldg = ldtp = nr) */
int jur_formod_device_ld(jur_model_t *m, long nr, double const *d_geom, long ldg, double *d_rad, double *d_tau, double *d_tp,
                         long ldtp, int *d_np, int *d_status, void *stream);
int jur_model_device(jur_model_t const *m);
int jur_model_nd(jur_model_t const *m);
void *jur_model_stream(jur_model_t const *m);
int *jur_model_status_word(jur_model_t const *m);
/* step sizes of the ray tracer and the altitude range of the atmosphere on the device (for cost estimates) */
void jur_model_cost_params(jur_model_t const *m, double *rayds, double *raydz, double *zmin, double *zmax);
/* device scratch of the model for nr rays laid out as jur_formod_host's image: geom[7][nr] | rad[nr][nd] | tau[nr][nd] |
 * tp[3][nr] doubles, np[nr] ints */
int jur_model_io(jur_model_t *m, long nr, double **d_io, int **d_io_np);

/* host tables (jur_tables.c) */
typedef struct {
  double t;
  int nu, cap;
  float *u, *eps;
} jur_curve_t;

typedef struct {
  double p;
  int nt;
  jur_curve_t cv[JUR_TBLNT];
} jur_level_t;

typedef struct {
  int np;                       /* 0 = no table                                 */
  jur_level_t *lv;              /* [np]                                         */
} jur_pair_t;

struct jur_tables {
  int ng, nd;
  jur_pair_t *pair;             /* [ng*nd]                                      */
  double *sr;                   /* [nd][JUR_TBLNS]                              */
  char *have_sr;                /* [nd]                                         */
  long ignored_rows;            /* rows dropped because a curve was full        */
};

/* flatten host tables into the CSR arrays of jur_view_t (malloc'ed) */
typedef struct {
  long nlevel, ncurve, nentry;
  int sorted;                   /* all axes and curves non-decreasing           */
  int strict;                   /* ... strictly increasing, curves as stored     */
  int max_pair_curves;
  jur_int2 *pair;
  long long *pair_e0;           /* [npair] first entry of the pair in ue */
  jur_lvl_t *lvl;
  jur_crv_t *crv;
  jur_ue_t *ue;
} jur_flat_t;
int  jur_tables_flatten(jur_tables_t const *tb, jur_flat_t *out);
void jur_flat_free(jur_flat_t *f);

void jur_tables_cache_filename(char *out, size_t len, ctl_t const *ctl);
int jur_chan_setup(jur_chan_t *ch, double nu, int window);
void jur_set_error(char const *fmt, ...);
int  jur_parse_number(char const **pp, double *out);   /* strtod-equivalent reader of the table files */

extern const double jur_ctm_blob[] __attribute__((visibility("hidden")));

#ifdef __cplusplus
}
#endif
#endif
