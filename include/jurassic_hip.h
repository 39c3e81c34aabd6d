/* jurassic_hip.h -- C-ABI of the MI355X forward-model library (libjurassic_hip.so).
 *
 * Two groups of entry points, all plain C, no C++/torch types:
 *
 * (1) DROP-IN symbols, exactly what the reference's host code binds:
 *       formod()         reference src/jurassic.h:515-518, body CPUdrivers.c:179-194
 *       formod_GPU()     reference src/GPUdrivers.cu:253-262 (declared CPUdrivers.c:153-155);
 *                        this is the object the reference links instead of GPUdrivers.o
 *       formod_pencil()  reference src/jurassic.h:526-530 (prototype only upstream)
 *     Same argument meaning, ownership and error behaviour as upstream: void
 *     return, a failure prints a message and terminates the process; tables are
 *     loaded from ${TBLBASE}_${nu}_${gas}.tab / .filt on first use and cached for
 *     the life of the process (jr_common.h:60-78).
 *
 * (2) ADDITIVE batched API (jur_*), for more than NR rays per call and for
 *     callers that already hold their arrays in device memory.  Returns 0 on
 *     success, a negative JUR_E* code otherwise; jur_last_error() has the text.
 */
#ifndef JURASSIC_HIP_H
#define JURASSIC_HIP_H

#include "jurassic_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- (1) drop-in ---------------------------------------------------------- */
void formod(ctl_t const *ctl, atm_t *atm, obs_t *obs);
void formod_GPU(ctl_t const *ctl, atm_t *atm, obs_t *obs);
void formod_pencil(ctl_t const *ctl, atm_t *atm, obs_t *obs, int const ir);
/* formod() plus the contribution of every emitter (the reference's `formod ... TASK contrib`) in one call: obs as
 * formod() leaves it; contrib[0 .. ng] (caller's array of ng + 1 obs_t) receive obs's geometry and tangent points and
 * the spectra of jur_formod_contrib_host's variants (contrib[g]: emitter g alone, contrib[ng]: the extinction alone) */
void formod_contrib(ctl_t const *ctl, atm_t *atm, obs_t *obs, obs_t *contrib);
/* field-of-view convolution of the radiances / transmittances in obs (jurassic.h:521, jurassic.c:214-258);
 * no-op when ctl->fov is "-"; host code */
void formod_fov(ctl_t const *ctl, obs_t *obs);

/* regridding of an atmosphere onto the points of another (jurassic.h:581-585, jurassic.c:675-683): dest->p, t, q, k
 * at dest's z / lon / lat from src by ctl->ip = 1 (one profile), 2 (the nearest two profiles of a satellite
 * track) or 3 (distance-weighted mean of a point cloud, ctl->cx / ctl->cz); GPU, device ctl->MPIlocalrank */
void intpol_atm(ctl_t *ctl, atm_t *atm_dest, atm_t *atm_src);

/* kernel() (reference jurassic.h:664, jurassic.c:812-857): forward-difference Jacobian of the finite radiances with
 * respect to the state elements inside the ctl->ret*_zmin/zmax windows, as ONE batched forward-model call on the GPU
 * (the difference quotients are formed on the device too); obs returns the unperturbed forward model.  The reference's
 * last argument is a gsl_matrix *: this library does not depend on GSL, jur_gsl_matrix_t restates that struct's layout
 * (gsl/gsl_matrix_double.h, unchanged since GSL 1.0: size1, size2, tda, data, block, owner) -- a caller that has GSL
 * passes its gsl_matrix * (same object), one that has not fills the first four fields.  size1 must be the number of
 * finite radiances of obs, size2 the state size (what obs2y / atm2x return upstream; jur_measurement_size /
 * jur_state_size here). */
typedef struct { size_t size1, size2, tda; double *data; void *block; int owner; } jur_gsl_matrix_t;
void kernel(ctl_t const *ctl, atm_t *atm, obs_t *obs, jur_gsl_matrix_t *k);

/* ---- (2) additive --------------------------------------------------------- */
enum {
  JUR_OK = 0,
  JUR_EINVAL = -1,    /* bad argument / unsupported control setting          */
  JUR_EIO = -2,       /* table or filter file problem                        */
  JUR_ENOMEM = -3,
  JUR_EHIP = -4,      /* HIP runtime error                                   */
  JUR_ENLOS = -5,     /* a line of sight needs >= NLOS points (jr_common.h:693) */
  JUR_ENODEV = -6     /* no usable GPU                                       */
};

char const *jur_last_error(void);

/* sizeof(ctl_t), sizeof(atm_t), sizeof(obs_t), ND, NG the library was built with */
void jur_abi_sizes(size_t out[5]);
/* C1, C2, P0, RE (reference jurassic.h:109-126) and the GSL 2.5 values of N_A, k_B, R (used at jr_common.h:330,
 * 450, 744) the library was built with */
void jur_abi_constants(double out[7]);

/* Host-side emissivity tables under construction. */
typedef struct jur_tables jur_tables_t;
jur_tables_t *jur_tables_new(int ng, int nd);
void jur_tables_free(jur_tables_t *tb);
/* Feed the rows (p [hPa], T [K], u [molec/cm^2], eps) of one (gas, channel)
 * table in file order; row acceptance follows reference jurassic.c:346-395. */
int jur_tables_feed_rows(jur_tables_t *tb, int ig, int id, long nrows,
                         double const *p, double const *t, double const *u, double const *eps);
/* Parse every ${tblbase}_${nu:%.4f}_${emitter}.tab named by ctl; missing files
 * leave that pair without table (transparent), as upstream.  Returns the number
 * of files found or a negative error. */
int jur_tables_read_ascii(jur_tables_t *tb, ctl_t const *ctl);
/* Filter function of one channel -> source-function table (jurassic.c:612-667). */
int jur_tables_set_filter(jur_tables_t *tb, int id, int n, double const *nu, double const *f);
int jur_tables_read_filters(jur_tables_t *tb, ctl_t const *ctl);
/* Compact binary cache of parsed tables + source functions (own format: text header naming
 * emitters and channels, then the flattened arrays and a checksum; ~8 bytes per table entry).
 * jur_tables_load: JUR_OK, JUR_EIO (no file) or JUR_EINVAL (other emitters/channels, damaged).
 * jur_model_create_from_files uses it under `bin.jurassic-hip-tables-g<ng>-d<nd>` in the
 * working directory as ctl->read_binary / ctl->write_binary ask (reference jurassic.c:312-320). */
int  jur_tables_save(jur_tables_t const *tb, ctl_t const *ctl, char const *path);
int  jur_tables_load(jur_tables_t **out, ctl_t const *ctl, char const *path);
void jur_tables_cache_filename(char *out, size_t len, ctl_t const *ctl);
/* FNV-1a over the flattened tables and source functions */
unsigned long long jur_tables_checksum(jur_tables_t const *tb);
/* number of stored (u,eps) entries, for reporting */
long jur_tables_entries(jur_tables_t const *tb);

/* A model = control settings + tables + per-channel continuum constants,
 * resident on one GPU (`device` = HIP device ordinal). */
typedef struct jur_model jur_model_t;
int  jur_model_create(jur_model_t **out, ctl_t const *ctl, jur_tables_t const *tb, int device);
/* convenience: tables + filters from the files ctl names */
int  jur_model_create_from_files(jur_model_t **out, ctl_t const *ctl, int device);
void jur_model_destroy(jur_model_t *m);

/* Upload the atmosphere (only atm->np points and ctl->ng gases travel).
 * Applies the hydrostatic adjustment first if ctl->hydz >= 0 -- on a private
 * copy; the caller's atm is not modified (GPU-path behaviour upstream,
 * GPUdrivers.cu:243).  An atmosphere identical to the one on the device is not
 * uploaded again.
 * Ordering: the upload waits for the model's last jur_formod_device call
 * (whose kernels may still read the old atmosphere) through an event of the
 * model's own that the call left on the caller's stream -- no handle of the
 * caller's is kept, the stream may have been destroyed since.  Device-entry
 * calls on other streams are chained to that one (see jur_formod_device);
 * launches of a captured graph are the caller's to synchronise. */
int  jur_model_set_atm(jur_model_t *m, atm_t const *atm);

/* Forward model for nr rays, host arrays.  geom[7] = {time, obsz, obslon,
 * obslat, vpz, vplon, vplat}, each [nr].  rad/tau are [nr][nd] (nd = ctl->nd,
 * channel fastest); rad is read first: channels that hold a non-finite value
 * on input come back NaN (jr_common.h:193-210).  tp[3] = {tpz, tplon, tplat},
 * each [nr].  np_out (optional) receives the number of LOS points per ray.
 * Pencil beams: a shape set with jur_model_set_fov is not applied by this entry, jur_formod_device, the contribution
 * entries or the drop-ins; their caller applies jur_fov_apply / jur_fov_apply_device. */
int  jur_formod_host(jur_model_t *m, long nr, double const *const geom[7],
                     double *rad, double *tau, double *const tp[3], int *np_out);

/* jur_formod_host moves arrays that lie in pinned host memory (these allocators, hipHostMalloc,
 * hipHostRegister) in place at PCIe speed and overlaps the transfers with the kernels; pageable arrays
 * are staged through a pinned image inside the model (threaded memcpy).  NULL on failure. */
void *jur_host_alloc(size_t bytes);
void  jur_host_free(void *p);

/* Same, all pointers in device memory of the model's GPU; work is enqueued on
 * `stream` (a hipStream_t, may be NULL) and the call returns without waiting.
 * d_geom is [7][nr], d_tp is [3][nr], d_np (optional) [nr].
 * d_status (optional, int[1]) is set non-zero on device if a ray overflowed NLOS.
 * Ordering between calls of ONE model: they share its workspace, so every call first lets its stream wait for an
 * event that the model's last device-entry call left behind its work, whichever stream that was on -- this entry on
 * `stream`; jur_formod_host, jur_formod_contrib_host, jur_kernel and jur_curtis_godson_host on the model's own stream.
 * Calls on different streams thus run in call order, one after the other (one model per stream overlaps).  While
 * `stream` is being captured into a graph the call neither waits nor leaves the event: launches of the graph are the
 * caller's to order against every other call of the model.  One host thread at a time per model. */
int  jur_formod_device(jur_model_t *m, long nr, double const *d_geom,
                       double *d_rad, double *d_tau, double *d_tp, int *d_np,
                       int *d_status, void *stream);

/* Contributions of the emitters: the call of jur_formod_host / jur_formod_device (rad, tau, tp, np the same doubles)
 * and, from its one ray trace and one table look-up, ng + 1 further spectra rad_c / tau_c [ng + 1][nr][nd] in the
 * caller's ray order:
 *   variant g < ng  the forward model on the atmosphere with q of every other gas and k of every window set to 0;
 *   variant ng      ... with every q set to 0 (the extinction alone).
 * The control block applies as it is (continua, write_bbt, hydz, refraction); every variant carries the NaN mask of
 * the input rad.  With ctl->hydz >= 0 and H2O the hydrostatic step's emitter (CTM_H2O on), zeroing q_H2O changes the
 * pressure profile: the variants other than H2O's are then traced on their own edited atmospheres (stacked as profile
 * slices, one further batched call) and the device entry waits for its stream before it returns. */
int  jur_formod_contrib_host(jur_model_t *m, long nr, double const *const geom[7], double *rad, double *tau,
                             double *const tp[3], int *np_out, double *rad_c, double *tau_c);
int  jur_formod_contrib_device(jur_model_t *m, long nr, double const *d_geom, double *d_rad, double *d_tau,
                               double *d_tp, int *d_np, int *d_status, double *d_rad_c, double *d_tau_c, void *stream);

/* ---- several GPUs in one process ------------------------------------------------------------------------------
 * The reference's device loop lives inside formod_GPU (GPUdrivers.cu:344-358: one OpenMP thread per device, every
 * device given the same package); SURVEY.md section 8e asks for "one host process, one stream set per device" with the
 * rays partitioned.  models[0 .. nmodel) are models of the same control block and tables, normally one per device
 * (several on one device are allowed: that is how a one-GPU box rehearses the path); each needs the atmosphere
 * (jur_models_set_atm).  Rays are dealt in CONTIGUOUS ranges whose boundaries equalise the estimated number of
 * line-of-sight points (jur_multi_balance: straight-line path through the atmosphere's altitude range in steps of
 * min(RAYDS, RAYDZ / |cos a|)), not the number of rays -- a tangent-height scan in its natural order has 122 .. 393
 * points per ray.  Results are the single-model results bit for bit.
 *
 * jur_formod_host_multi: host arrays as jur_formod_host; one host thread per model, every share written straight
 *   into the caller's arrays (pinned arrays move in place), no gather.
 * jur_formod_device_multi: all arrays in device memory of models[0]'s GPU (layout as jur_formod_device).  Share 0 is
 *   computed in place on `stream`; the others travel to their model's device and back with hipMemcpyPeerAsync on that
 *   model's own stream (xGMI between the GPUs of a node), and `stream` waits for them: no host synchronisation.
 *   bounds[0 .. nmodel] (optional, NULL: equal ray counts): share k = rays [bounds[k], bounds[k+1]), e.g. from
 *   jur_multi_balance when the geometry is known on the host.  d_status (optional) is int[nmodel], one word per share. */
int  jur_multi_balance(jur_model_t const *m, long nr, double const *const geom[7], int nparts, long *bounds);
/* The same without a model or a GPU (host arithmetic only): the estimated number of LOS points of every ray from the
 * tracer's step sizes (ctl->rayds, ctl->raydz) and the altitude range [zmin, zmax] of the atmosphere, and the balanced
 * boundaries from it -- what a launcher that deals a SORTED observation set to one process per GPU needs
 * (jurassic_hip/shard.py: balanced_ranges). */
int  jur_estimate_los_points(double rayds, double raydz, double zmin, double zmax, long nr, double const *const geom[7], double *points);
int  jur_balance_rays(double rayds, double raydz, double zmin, double zmax, long nr, double const *const geom[7], int nparts, long *bounds);
int  jur_models_set_atm(jur_model_t *const models[], int nmodel, atm_t const *atm);
int  jur_formod_host_multi(jur_model_t *const models[], int nmodel, long nr, double const *const geom[7],
                           double *rad, double *tau, double *const tp[3], int *np_out);
int  jur_formod_device_multi(jur_model_t *const models[], int nmodel, long nr, long const *bounds, double const *d_geom,
                             double *d_rad, double *d_tau, double *d_tp, int *d_np, int *d_status, void *stream);

/* Retrieval support (reference kernel(), jurassic.c:812-857; state/measurement
 * vectors as atm2x/obs2y, :1491-1541): forward-difference Jacobian dy/dx of the
 * finite radiances with respect to the atmosphere values inside the
 * ctl->ret{p,t,q,k}_zmin/zmax windows, evaluated as one batched forward-model
 * call (n+1 stacked atmospheres) whose difference quotients are formed on the device.  k is row-major
 * [jur_measurement_size][jur_state_size];
 * obs returns the unperturbed result.  The reference's signature takes a gsl_matrix;
 * bind with k = matrix->data when matrix->tda == matrix->size2.
 * The model holds `atm` afterwards (as after jur_model_set_atm) -- after an error return (JUR_ENLOS, ...) too; if
 * that upload fails, it holds no atmosphere and refuses the next call.
 * jur_kernel and kernel() difference pencil beams: a shape set with jur_model_set_fov is not applied; the caller applies
 * jur_fov_apply to the columns there (or uses the scene entries, which honour it). */
size_t jur_state_size(jur_model_t const *m, atm_t const *atm);
size_t jur_measurement_size(jur_model_t const *m, obs_t const *obs);
int    jur_kernel(jur_model_t *m, atm_t const *atm, obs_t *obs, double *k, size_t mrows, size_t ncols);

/* The Jacobian of a whole scene as per-ray blocks, for any number of rays.  A ray is traced through the slice
 * [first, first + len) of the atmosphere that locate_atm hands it (jr_common.h:127-154) and through nothing else, so
 * its rows of jur_kernel's matrix are exactly 0 outside the state elements of that slice: only those are computed.
 *
 * jur_scene_layout (host arithmetic, no GPU): slice of every ray with time stamp time[r], and where its block starts:
 *   width[r] = number of state elements (atm2x order, ctl->ret*_zmin/zmax) whose point lies in the slice, 0 for a slice
 *   of fewer than 2 points; rowptr[0] = 0, rowptr[r + 1] = rowptr[r] + width[r]; rowptr is [nr + 1].
 * jur_scene_columns: the global state indices (columns of jur_kernel's matrix) of the slice, ascending; returns their
 *   number (cols may be NULL to count) or JUR_EINVAL.  Slices are pairs (first, len), not profiles: a lone end point
 *   joins its neighbour's slice, and a ray time stamp may match no profile.
 * jur_kernel_scene_host: geom, rad (read first for the NaN mask), tau, tp, np_out as jur_formod_host; they return the
 *   unperturbed forward model, the doubles of jur_formod_host on `atm`.  k holds rowptr[nr] * nd doubles: the block of
 *   ray r starts at k + rowptr[r] * nd, is laid out [nd][width[r]] with the columns of jur_scene_columns, and entry
 *   (id, e) is (y1 - y0) / h with the reference's step h (jurassic.c:833-836) -- the doubles of jur_kernel's entry.
 *   A channel masked on input gives a row of NaN; rows are never compacted.  rowptr must be jur_scene_layout's
 *   (JUR_EINVAL otherwise).  The perturbed slices, the replicated rays and the quotients are made on the device; rays
 *   are taken in contiguous passes whose replicated count (width + 1 per ray) stays within max_rays_per_pass (0: a
 *   sixteenth of what the stacked slices leave of the model's workspace budget, 4096 at least; a ray beyond it alone
 *   goes alone); the blocks of a pass are copied straight into k
 *   (pinned memory from jur_host_alloc travels fastest).
 *   JUR_EINVAL, with a message: ctl->hydz >= 0 (the hydrostatic adjustment treats all points as one profile, so every
 *   p, T or H2O element moves every pressure and there are no blocks: use jur_kernel); time stamps of atm not
 *   ascending; atm->np outside 2..JUR_NP.  JUR_ENOMEM when the stacked slices exceed half the workspace budget (call
 *   with the rays of fewer slices).  nr == 0 is JUR_OK; a state of zero elements gives the forward model alone.
 *   The model holds `atm` afterwards, after a refusal or an error too (as jur_kernel).
 * jur_model_last_scene_ms: the share of the stacking, replication and quotient kernels in the launches timed since
 *   the last call (after jur_model_last_kernel_ms, which collects the events). */
int  jur_scene_layout(ctl_t const *ctl, atm_t const *atm, long nr, double const *time, int *first, int *len, long *rowptr);
long jur_scene_columns(ctl_t const *ctl, atm_t const *atm, int first, int len, long *cols);
int  jur_kernel_scene_host(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double *rad, double *tau,
                           double *const tp[3], int *np_out, long const *rowptr, double *k, long max_rays_per_pass);
int  jur_model_last_scene_ms(jur_model_t *m, double *out_ms, long *out_launches);

/* The Gauss-Newton normal equations of a scene per slice, accumulated on the device from the blocks of
 * jur_kernel_scene_host while they lie there: for every distinct slice s of the scene, over its live measurements
 * (r, id), with F the unperturbed radiance the call returns in rad and K_r the block of ray r,
 *   A_s[i][j] = sum weight * K_r[id][i] * K_r[id][j],  b_s[i] = sum weight * K_r[id][i] * (y - F),
 *   cost[s] = sum weight * (y - F)^2,  nlive[s] = number of terms.
 *
 * jur_scene_slices (host arithmetic, no GPU): the distinct slices (first, len) of width > 0 among the rays with time
 *   stamps time[r], in the order the rays first meet them; rays with different time stamps can share one.  sid[r] is the
 *   slice of ray r, -1 for a ray of width 0; wptr and aptr [nslice + 1] are the running sums of the widths w_s and of
 *   w_s^2.  Any output may be NULL: a first call counts.  Returns nslice, or what jur_scene_layout refuses, as there.
 * jur_scene_elements: jur_scene_columns plus the quantity iq (0 p, 1 T, 2 + g q, 2 + ng + w k) and the atmosphere point
 *   ip of every element (any output may be NULL): what writes a solved step back into an atm_t.
 * jur_normal_scene_host: geom, rad (read first for the NaN mask), tau, tp, np_out, rowptr and max_rays_per_pass as
 *   jur_kernel_scene_host, with the same doubles out and the same refusals.  y and weight are [nr][nd]: the
 *   measurements and the diagonal of the inverse of their covariance, 1 / sigma^2.  A weight that is negative or not
 *   finite gives JUR_EINVAL.  A measurement is live when its channel is not masked on input (any non-finite rad masks), y is finite, its weight
 *   is > 0 and its ray has a slice; one that is not contributes nothing (no 0 * NaN is formed).
 *   A holds aptr[nslice] doubles, A_s at A + aptr[s] laid out [w_s][w_s], full, its two triangles bit-identical;
 *   b holds wptr[nslice] doubles, b_s at b + wptr[s]; cost and nlive hold nslice entries, all laid out by
 *   jur_scene_slices of the same rays.  Every sum runs in ascending ray order and within a ray in ascending channel
 *   order, without atomics, in accumulators that stay on the device across the passes: the results depend neither on
 *   max_rays_per_pass nor on k nor on where the rays of a slice sit in the call.
 *   k may be NULL: no block leaves the device then.  Otherwise it receives the blocks of jur_kernel_scene_host.
 *   nr == 0 and a state of zero elements are JUR_OK with nslice == 0: nothing is written to A, b, cost, nlive.
 *   JUR_ENOMEM when the normal matrices do not fit beside the stacked slices in half the workspace budget.
 *   The kernel's time counts into jur_model_last_scene_ms.  The model holds `atm` afterwards, after an error too. */
long jur_scene_slices(ctl_t const *ctl, atm_t const *atm, long nr, double const *time, int *sid, int *sfirst, int *slen,
                      long *wptr, long *aptr);
long jur_scene_elements(ctl_t const *ctl, atm_t const *atm, int first, int len, long *cols, int *iq, int *ip);
int  jur_normal_scene_host(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double *rad, double *tau,
                           double *const tp[3], int *np_out, long const *rowptr, double const *y, double const *weight,
                           double *A, double *b, double *cost, long *nlive, double *k, long max_rays_per_pass);

/* The Levenberg-Marquardt step of every slice: a batched, ragged Cholesky solve on the device of the damped, optionally
 * regularised normal equations, for nlam dampings in one call.  One system (slice s, width w, damping lam), with
 * r = prior_ivar (inverse a-priori variances) and d = prior_dx (a-priori minus current state), both 0 without a prior:
 *   D_i = A_ii + r_i;  element i is live when D_i > 0 (anything else, NaN included, is dead)
 *   s_i = D_i (JUR_DAMP_MARQUARDT) or r_i (JUR_DAMP_PRIOR, the damping (1 + lam) Sa^-1)
 *   M_ii = fma(lam, s_i, D_i),  M_ij = A_ij (i > j, both live),  g_i = fma(r_i, d_i, b_i)
 *   M = L L^T on the live elements, L z = g, L^T dx = z;  pred = sum dx_i * (g_i + lam s_i dx_i),
 * pred being the decrease of the cost sum weight (y - F)^2 + sum r (x - xa)^2 that the linearised model predicts for the
 * step.  Only the diagonal and the lower triangle of A_s are read.  A dead element's row and column are ignored, its dx
 * is +0.0 and in L its diagonal is 1 and the rest of its row and column 0 (in the A_s of jur_normal_scene_host a zero
 * diagonal means a zero row, so nothing is lost).  A pivot that is not > 0 just before its square root (NaN included)
 * breaks the system down: status = 1 + the index in the slice of that column, dx_s all +0.0, pred 0, L_s all zeros; no
 * other system is affected.  Otherwise status = 0.
 *
 * jur_solve_in_t: lam is [nlam][nslice], each >= 0 and finite; prior_ivar (each >= 0 and finite) and prior_dx (finite)
 *   hold wptr[nslice] doubles each and are given both or neither; JUR_DAMP_PRIOR needs them.
 * jur_solve_out_t: dx [nlam][wptr[nslice]], pred and status [nlam][nslice]; L is optional, [nlam][aptr[nslice]], L_s laid
 *   out as A_s with exact zeros above the diagonal.  The caller owns all of them.
 * Every double of a system depends on its own inputs and on w alone: not on the number or the order of the systems of
 *   the call, not on nlam, not on max_rays_per_pass, not on which of the two entries was called.  No atomics; every sum
 *   runs in an order fixed by w.
 * jur_solve_slices_host: systems the caller holds (the re-solve after a rejected step): A_s at A + aptr[s], [w_s][w_s],
 *   aptr the running sum of w_s^2 with w_s = wptr[s + 1] - wptr[s]; b_s at b + wptr[s].  The model supplies the device
 *   and the stream and the call is ordered against the model's other calls; the model's atmosphere and workspace are
 *   not touched.  nslice == 0 is JUR_OK and writes nothing.
 * jur_step_scene_host: jur_normal_scene_host followed by the solve on accumulators that stay on the device: every
 *   argument of that entry as there, with the same doubles out and the same refusals; A, b and k may be NULL and then
 *   never leave the device.  The layout of dx, pred, status, L is that of jur_scene_slices of the same rays.
 * JUR_EINVAL, with a message that names the slice and the damping or the element: nlam < 1; an unknown mode; a lam that
 *   is negative or not finite; a prior_ivar that is negative or not finite; a prior_dx that is not finite; one of the
 *   prior pair without the other; JUR_DAMP_PRIOR without a prior; NULL among lam, dx, pred, status; wptr not ascending.
 * JUR_ENOMEM (jur_step_scene_host, before anything is launched) when the accumulators and the solver scratch -- one
 *   more copy of the matrices, the vectors of one damping and the outputs of all -- do not fit beside the stacked
 *   slices in half the workspace budget.  JUR_EHIP when a launch fails.
 * The kernel's time counts into jur_model_last_scene_ms. */
enum { JUR_DAMP_MARQUARDT = 0, JUR_DAMP_PRIOR = 1 };
typedef struct {
  int nlam, mode;
  double const *lam;                      /* [nlam][nslice] */
  double const *prior_ivar, *prior_dx;    /* [wptr[nslice]] each; both or neither */
} jur_solve_in_t;
typedef struct {
  double *dx;                             /* [nlam][wptr[nslice]] */
  double *pred;                           /* [nlam][nslice] */
  int *status;                            /* [nlam][nslice] */
  double *L;                              /* optional, [nlam][aptr[nslice]], rows as A_s, strict upper 0 */
} jur_solve_out_t;
int  jur_solve_slices_host(jur_model_t *m, long nslice, long const *wptr, double const *A, double const *b,
                           jur_solve_in_t const *in, jur_solve_out_t const *out);
int  jur_step_scene_host(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double *rad, double *tau,
                         double *const tp[3], int *np_out, long const *rowptr, double const *y, double const *weight,
                         jur_solve_in_t const *in, jur_solve_out_t const *out,
                         double *A, double *b, double *cost, long *nlive, double *k, long max_rays_per_pass);

/* Retrieval of a scene: iterated Levenberg-Marquardt with trial steps, slice by slice, on the device.
 * All arrays follow the layout of jur_scene_slices of the call's rays; the entries refuse what jur_step_scene_host refuses
 * (hydz >= 0, time stamps that are not ascending, np outside 2..JUR_NP, a rowptr that is not jur_scene_layout's).
 *
 * jur_trial_scene_host: the cost of every slice under ntrial candidate steps, forward only.  For trial t and slice s the
 *   atmosphere is atm with every element e of s set to x_e + dx[t][e] (one IEEE addition), formed on the device in a copy
 *   of the slice's points under a time stamp of its own; the rays of s are traced through it, ntrial rays per ray, and
 *   cost[t][s] is the chain of jur_normal_scene_host's cost (acc = fma(weight * d, d, acc), d = y - F, ascending rays, then
 *   ascending channels) over the live measurements (rad_in's NaN mask, y finite, weight > 0, a ray with a slice): bit for
 *   bit what jur_normal_scene_host returns on the atmosphere with the step written back.  A trial radiance that is not
 *   finite makes that one cost NaN.  prior[t][s] = sum_e r_e (xa_e - (x_e + dx[t][e]))^2 as separately rounded operations
 *   (difference, r * d, * d, sum; ascending e), +0.0 without a prior.  No atomics: every double depends on its slice's
 *   inputs alone, not on the other slices, ntrial or the passes (max_rays_per_pass caps the replicated rays, ntrial per
 *   ray).  JUR_EINVAL: ntrial outside 1..64, a dx that is not finite, half a prior.  JUR_ENOMEM, before anything is
 *   launched, when the trial copies and accumulators do not fit into half the workspace budget.  The model holds atm
 *   afterwards.
 * jur_retrieve_decide: the accept/reject policy of one iteration, host arithmetic, no GPU.  Per slice with
 *   state == JUR_RET_ACTIVE: the candidates are the l with status[l][s] == 0 and a Jt[l][s] that is not NaN; best is the
 *   one with the smallest Jt (ties: the smallest l), -1 without candidates; accept = best >= 0 && Jt[best] < J (strict).
 *   Accepted: lam = lamt[best], and state = JUR_RET_CONVERGED if J - Jt[best] <= tol * J.  Rejected: state =
 *   JUR_RET_STALLED if lam == lam_max on entry, otherwise lam = min(lam * fac_max, lam_max).  Other slices are left
 *   alone, with best = accept = -1.
 * jur_retrieve_scene_host: the loop.  Per iteration, for the slices still active: the body of jur_step_scene_host on the
 *   current state with the dampings lamt[l][s] = min(max(lam_s * fac[l], lam_min), lam_max) and prior_dx = xa - x formed
 *   on the device; J = cost + prior; the trial pass on the nlam steps where they lie; jur_retrieve_decide on the scalars
 *   brought home; x += dx[best] for the accepted slices in the base rows on the device.  A slice that is no longer active
 *   has its rays in no later pass; what is still active after max_iter becomes JUR_RET_MAXITER.  Geometry, mask, y,
 *   weight, prior and first guess go up once; per iteration the scalars per slice and damping come home and the dampings
 *   and choices go up (and, when slices have ended, the list of the remaining rays); x and the forward results come home
 *   once.  atm_ret is a copy of atm0 with the retrieved elements replaced (it may be atm0 itself; written only on
 *   success); rad, tau, tp, np_out are the doubles of jur_formod_host on atm_ret (rad in: the NaN mask), and the model
 *   holds atm_ret.  On any error (JUR_ENLOS from a trial ray included, unless jur_model_set_scene_overflow isolates such
 *   rays: see there) the model holds atm0 and atm_ret is untouched.
 *   The slices of a scene must be disjoint in atmosphere points (JUR_EINVAL names the two that are not).
 * The kernels' time counts into jur_model_last_scene_ms. */
int  jur_trial_scene_host(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double const *rad_in,
                          long const *rowptr, double const *y, double const *weight,
                          int ntrial, double const *dx,          /* [ntrial][wptr[nslice]] */
                          double const *prior_ivar, double const *prior_xa,   /* [wptr[nslice]] each; both or neither */
                          double *cost, double *prior,           /* [ntrial][nslice] each */
                          long max_rays_per_pass);
enum { JUR_RET_ACTIVE = 0, JUR_RET_CONVERGED = 1, JUR_RET_STALLED = 2, JUR_RET_MAXITER = 3 };
int  jur_retrieve_decide(int nlam, long nslice, double tol, double lam_max, double fac_max,
                         double const *J, double const *Jt, double const *lamt, int const *status, /* [nslice]; [nlam][nslice] x 3 */
                         double *lam, int *state,               /* [nslice] in/out */
                         int *best, int *accept);               /* [nslice] out; -1 for a slice that is not ACTIVE */
typedef struct {
  int max_iter, nlam, mode;            /* >= 1; 1..8; JUR_DAMP_* */
  double const *fac;                   /* [nlam] each > 0 and finite, at least one > 1 */
  double lam0, lam_min, lam_max, tol;  /* 0 < lam_min <= lam0 <= lam_max, all finite; tol >= 0 finite */
  double const *prior_ivar, *prior_xa; /* [wptr[nslice]]; both or neither; JUR_DAMP_PRIOR needs them */
} jur_retrieve_in_t;
typedef struct {
  double *x, *lam, *cost, *prior;      /* final: [wptr[nslice]], [nslice] x 3 (cost, prior: of the state x) */
  long *nlive; int *state, *iters;     /* [nslice] */
  /* optional history, all or none: */
  double *h_cost, *h_prior;            /* [max_iter][nslice] at the iteration's start (a slice that has ended: its last) */
  double *h_lam, *h_tcost, *h_tprior;  /* [max_iter][nlam][nslice]; NaN where the slice took no part */
  int *h_status;                       /* [max_iter][nlam][nslice]; -1 where the slice took no part (JUR_TRIAL_OVERFLOW: see jur_model_set_scene_overflow) */
  int *h_best, *h_accept;              /* [max_iter][nslice]; -1 where the slice took no part */
  long *h_work;                        /* [max_iter][2] replicated rays of the Jacobian passes, of the trial passes */
} jur_retrieve_out_t;
int  jur_retrieve_scene_host(jur_model_t *m, atm_t const *atm0, atm_t *atm_ret, long nr, double const *const geom[7],
                             double *rad, double *tau, double *const tp[3], int *np_out, long const *rowptr,
                             double const *y, double const *weight, jur_retrieve_in_t const *in,
                             jur_retrieve_out_t const *out, long max_rays_per_pass);

/* Posterior diagnostics of the slices: covariance, averaging kernel, degrees of freedom, errors, on the device.
 * One system (slice s, width w), with r = prior_ivar (all 0 without a prior): D_i = A_ii + r_i, element i live when
 * D_i > 0 (anything else, NaN included, is dead) -- the solve's rule; on the live elements M = A + diag(r) = L L^T, the
 * solve's M at lam = 0 (no damping).  Only the diagonal and the lower triangle of A_s are read.
 *   S = M^-1              posterior covariance, [w][w], full, its two triangles bit-identical
 *   AVK = S A             averaging kernel, [w][w], row i the response of retrieved element i (a product, not
 *                         I - S diag(r))
 *   avk_diag_i = AVK_ii;  dofs[s] = sum_i AVK_ii
 *   sigma_i = sqrt(S_ii);  sigma_noise_i = sqrt(max(sum_j AVK_ij S_ji, 0)), the diagonal of S A S;
 *   sigma_smooth_i = sqrt(sum_j S_ij^2 r_j), the diagonal of S diag(r) S
 * A dead element has its row and column of S and AVK +0.0, its sigmas and avk_diag +0.0, and adds nothing to dofs.  A
 * pivot that is not > 0 gives status[s] = 1 + its column as in the solve; every output of that system is +0.0 then and
 * no other system is affected.  Otherwise status[s] = 0.  A system of width 0 writes dofs = 0, status = 0.
 * Every double of a system depends on its own inputs and on w alone: not on the number or the order of the systems of
 *   the call, not on which of the two entries was called, not on max_rays_per_pass, not on whether S or avk were asked
 *   for.  No atomics; every sum runs in an order fixed by w.
 * jur_diag_out_t: sigma, sigma_noise, sigma_smooth, avk_diag [wptr[nslice]] and dofs, status [nslice] are required; S
 *   and avk are optional, [aptr[nslice]] each, laid out as A_s.  The caller owns all of them.
 * jur_diagnose_slices_host: systems the caller holds, laid out as for jur_solve_slices_host and under its contract (the
 *   model supplies device and stream; its atmosphere and workspace are not touched; nslice == 0 is JUR_OK and writes
 *   nothing).
 * jur_diagnose_scene_host: jur_normal_scene_host on `atm` -- the same doubles out, the same refusals; A, b, cost, nlive
 *   and k may each be NULL and then never leave the device -- followed by the diagnostics on the accumulators where they
 *   lie.  The layout is that of jur_scene_slices of the same rays.  Meant to be called once on the atm_ret of
 *   jur_retrieve_scene_host, with that call's prior_ivar.  The model holds `atm` afterwards.
 * JUR_EINVAL with a message naming the slice or the element: a required output that is NULL; wptr that does not ascend;
 *   a prior_ivar that is negative or not finite.  JUR_ENOMEM (jur_diagnose_scene_host, before anything is launched) when
 *   the factor, S, AVK and the vectors do not fit beside the normal matrices and the stacked slices in half the
 *   workspace budget.  JUR_EHIP when a launch fails.  The kernels' time counts into jur_model_last_scene_ms.
 * jur_avk_summary (host arithmetic, no GPU): what is read off one slice's averaging kernel avk [w][w], with the elements
 *   of jur_scene_elements(ctl, atm, first, len, ...), quantity iq and point ip each:
 *   dofs_q[q] = sum of AVK_ii over the elements of quantity q (2 + ng + nw entries);
 *   area_i = sum_j AVK_ij over the j of i's quantity, ascending (near 1: the measurement drives the element);
 *   resolution_i = dz_i / AVK_ii, dz_i half the altitude distance between the neighbouring retrieved points of i's
 *   quantity in the slice, the full distance to the one neighbour at either end, 0 for a lone element; +inf where AVK_ii
 *   is not > 0.  JUR_EINVAL for a slice outside the atmosphere or a NULL argument. */
typedef struct {
  double *sigma, *sigma_noise, *sigma_smooth, *avk_diag;  /* [wptr[nslice]] each, required */
  double *dofs; int *status;                              /* [nslice], required */
  double *S, *avk;                                        /* optional, [aptr[nslice]] each, laid out as A_s */
} jur_diag_out_t;
int  jur_diagnose_slices_host(jur_model_t *m, long nslice, long const *wptr, double const *A,
                              double const *prior_ivar /* or NULL */, jur_diag_out_t const *out);
int  jur_diagnose_scene_host(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double *rad, double *tau,
                             double *const tp[3], int *np_out, long const *rowptr, double const *y, double const *weight,
                             double const *prior_ivar, jur_diag_out_t const *out,
                             double *A, double *b, double *cost, long *nlive, double *k, long max_rays_per_pass);
int  jur_avk_summary(ctl_t const *ctl, atm_t const *atm, int first, int len, double const *avk /* [w][w] */,
                     double *dofs_q /* [2 + ng + nw] */, double *area /* [w] */, double *resolution /* [w] */);

/* Gain matrix and per-source error budget of the slices, on the device (upstream's matrix_gain.tab, atm_err_noise.tab and
 * atm_err_formod.tab).  G = S K^T Se^-1 maps a perturbation of the measurements into the state: dx = G dy.
 * Measurements and weights.  The measurements (r, id) of slice s (width w) are those of the rays with sid[r] == s, in
 *   ascending ray order and within a ray in ascending channel order.  The effective weight omega of a measurement is
 *   weight[r][id] where the measurement is live and 0 otherwise; live is jur_normal_scene_host's rule (input radiance --
 *   with a field of view the effective mask --, F and y finite, weight > 0, and the ray has a slice).
 * S_s is the posterior covariance of jur_diagnose_scene_host in every configuration (with the model's full prior
 *   precision where one is set).  Element j is dead when S_jj is not > 0 (NaN included).
 * The gain.  G_s[i][(r, id)] = omega * c, c the chain over j = 0 .. w - 1 ascending from +0.0 of fma(S_ij, K_r[id][j], c).
 *   A dead j is skipped: its block entry is never multiplied, so a NaN there goes nowhere.  A dead i gives +0.0.  A
 *   measurement that is not live gives a row of +0.0 and its block row is never read (a masked channel holds NaN there).
 *   A system whose diagnostics broke down (status != 0) gives +0.0 throughout.
 * Layout.  The gain block of ray r lies at gain + rowptr[r] * nd as [nd][width]: where and how jur_kernel_scene_host puts
 *   K_r, so G is stored measurement-major like the blocks (entry (id, i) of the block is G_s[i][(r, id)]).
 * Budget.  For component c < ncomp with variances var[c][r][id]:
 *   sigma_comp[c][wptr[s] + i] = sqrt(q), q the chain over the live measurements of s, ascending, from +0.0 of
 *   fma(g * g, var, q), g = G_s[i][(r, id)], g * g rounded first.  var is read on live measurements only; a value there
 *   that is negative or not finite is JUR_EINVAL naming component, ray and channel, before anything is launched (the
 *   scene entry decides this before the forward model has run: from the input mask, y, the weight and the slice).
 *   ncomp is 0 to 8; 0 means the gain only.  out->gain is optional, out->sigma_comp required when ncomp > 0.
 * Every double depends on its own slice's inputs and on w alone: not on the other slices, their order,
 *   max_rays_per_pass or the entry called.  No atomics; every chain is fixed by the slice.
 * jur_gain_slices_host: systems and blocks the caller holds, under the contract of jur_diagnose_slices_host (the model
 *   supplies device and stream; its atmosphere and workspace are not touched).  S as jur_diagnose_slices_host lays it out,
 *   status its breakdowns or NULL (all 0), k and rowptr as jur_kernel_scene_host's, sid[r] the slice of ray r (-1: none;
 *   the width of a ray must be that of its slice), weight_eff omega directly: anything not > 0 is "not live".  nslice == 0
 *   or nr == 0 is JUR_OK and writes nothing.
 * jur_gain_scene_host: jur_diagnose_scene_host -- rad, tau, tp, np_out, A, b, cost, nlive, k and every field of diag are
 *   that entry's bit for bit, and its refusals are the same -- with the blocks of all rays kept in the device slab (with a
 *   field of view the convolved ones), the effective weights formed on the device, and the two kernels run once S exists.
 *   The gain is written to an array of its own beside the retained blocks, never over them: k and gain may both be asked
 *   for.  Only what was asked for is copied home.  JUR_ENOMEM before anything is launched when the retained blocks, the
 *   gain and the budget's arrays do not fit beside everything else in half the workspace budget.  The model holds atm
 *   afterwards, after an error too; the kernels' time counts into jur_model_last_scene_ms.
 * jur_error_components (host arithmetic, no GPU; upstream's set_cov_meas): var[0][r][id] = err_noise[id]^2, var[1][r][id]
 *   = (err_formod[id] / 100 * y[r][id])^2, weight = 1 / (their sum) where that sum is finite and > 0; otherwise weight = 0
 *   and both variances +0.0 (a y that is not finite among them).  JUR_EINVAL for a negative or non-finite err_*. */
typedef struct { int ncomp; double const *var; /* [ncomp][nr][nd] */ } jur_gain_in_t;
typedef struct {
  double *gain;                 /* optional, [rowptr[nr] * nd], laid out as the blocks */
  double *sigma_comp;           /* [ncomp][wptr[nslice]], required when ncomp > 0 */
} jur_gain_out_t;
int  jur_gain_slices_host(jur_model_t *m, long nslice, long const *wptr, double const *S, int const *status /* or NULL */,
                          long nr, int nd, long const *rowptr, int const *sid, double const *k, double const *weight_eff,
                          jur_gain_in_t const *in, jur_gain_out_t const *out);
int  jur_gain_scene_host(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double *rad, double *tau,
                         double *const tp[3], int *np_out, long const *rowptr, double const *y, double const *weight,
                         double const *prior_ivar, jur_diag_out_t const *diag, jur_gain_in_t const *in, jur_gain_out_t const *out,
                         double *A, double *b, double *cost, long *nlive, double *k, long max_rays_per_pass);
int  jur_error_components(int nd, long nr, double const *y, double const *err_noise /* [nd] */, double const *err_formod /* [nd], per cent */,
                          double *var /* [2][nr][nd]: noise, formod */, double *weight /* [nr][nd] */);

/* Parameter errors of the slices, on the device: the error of quantities b that are not retrieved (a temperature profile
 * under a trace-gas retrieval, an interfering gas, the pressure at the reference level, an extinction) reaches the
 * measurements through their Jacobian K_b, fully correlated across the channels and rays of a slice, and the state
 * through C_s = G_s^T K_b,s = dx^/db, the cross-state matrix of slice s ([w_s][wb_s]); its covariance in the state is
 * C_s Sigma_b C_s^T.  With K_b = K, C_s is the averaging kernel.
 * Inputs.  sid, wptr, rowptr, gain and weight_eff are what jur_gain_slices_host takes and writes for the retrieved state.
 *   kb and rowptr_b are blocks of jur_kernel_scene_host on the same rays under other retrieval windows (with a field of
 *   view or the hydrostatic balance set, the convolved or balanced ones): the block of ray r lies at kb + rowptr_b[r] * nd
 *   as [nd][wb].  wb_s is the width in rowptr_b of the rays of slice s (0 for a slice without rays), bwptr its running
 *   sum, cptr and bbptr the running sums of w_s * wb_s and wb_s^2 (jur_param_layout makes the three).  The width in
 *   rowptr_b of a ray without a slice is not looked at.
 * Measurements.  As jur_gain_slices_host: the rays with sid[r] == s ascending, the channels of a ray ascending; a
 *   measurement is live exactly when its weight_eff > 0.  A row that is not live is never read, in gain or in kb (kb
 *   holds NaN on masked channels).
 * The cross-state matrix.  C_s[i][j] = c, the chain over the live measurements m of s, ascending, from +0.0 of
 *   fma(G_m,i, Kb_m,j, c).  A dead state element has a zero gain column and so a row of +0.0 -- or of NaN where column j
 *   is: a NaN in a live row of kb reaches column j of that slice's C, all of it, and nothing else.  A slice with wb_s == 0
 *   has an empty C_s and a sigma_param of +0.0.
 * The budget.  Component c < nvar is diagonal, Sigma = diag(var[c][bwptr[s] + j]): q_i is the chain over j = 0 .. wb_s - 1
 *   ascending from +0.0 of fma(C_ij * C_ij, var_j, q), the square rounded first.  Component nvar + c, c < ncov, is full,
 *   Sigma_s = cov[c] at bbptr[s] as [wb_s][wb_s], of which the diagonal and the lower triangle are read (Sigma_jl for l > j
 *   is read as Sigma_lj): t_j is the chain over l ascending from +0.0 of fma(Sigma_jl, C_il, t), then q_i the chain over j
 *   ascending from +0.0 of fma(C_ij, t_j, q).  sigma_param[c][wptr[s] + i] = sqrt(q_i) where q_i > 0, NaN where q_i is
 *   NaN, +0.0 otherwise (a Sigma that is not positive semidefinite can give q_i < 0).  Messages count the components as
 *   sigma_param does: the diagonal ones first.
 * Every double depends on its own slice's inputs, w_s and wb_s alone: not on the other slices, their order, where the
 *   rays of a slice sit in the call, which components accompany it or whether C was asked for.  No atomics, no
 *   measurement chain split across workgroups, no MFMA.
 * jur_param_slices_host: under the contract of jur_gain_slices_host (the model supplies device and stream; its atmosphere
 *   and workspace are not touched; ordered against the model's other calls as that entry is).  nslice == 0 or nr == 0 is
 *   JUR_OK and writes nothing.  out->C is optional, out->sigma_param required when nvar + ncov > 0.  JUR_EINVAL, naming
 *   slice, ray, component or element, before anything is launched, for: a required pointer that is NULL; nvar, ncov
 *   negative or nvar + ncov > 8; wptr or bwptr not an ascending running sum from 0; a ray whose width in rowptr is not
 *   that of its slice; two rays of one slice with different widths in rowptr_b; a bwptr that does not agree with those
 *   widths; a var that is negative or not finite; an entry of cov that is read and not finite; a negative diagonal of
 *   cov.  JUR_ENOMEM, JUR_EHIP as jur_gain_slices_host.
 * jur_param_layout (host arithmetic, no GPU): bwptr, cptr, bbptr [nslice + 1] from the widths; any of the three may be
 *   NULL (a first call counts).  Returns cptr[nslice], or JUR_EINVAL with the layout refusals above. */
typedef struct {
  int nvar, ncov;            /* nvar + ncov in 0..8 */
  double const *var;         /* [nvar][bwptr[nslice]]   diagonal parameter covariances */
  double const *cov;         /* [ncov][bbptr[nslice]]   full ones, Sigma_s at bbptr[s], [wb_s][wb_s]; diagonal and lower triangle read */
} jur_param_in_t;
typedef struct {
  double *C;                 /* optional, [cptr[nslice]]: C_s at cptr[s], [w_s][wb_s] row-major */
  double *sigma_param;       /* [nvar + ncov][wptr[nslice]], the var components first; required when nvar + ncov > 0 */
} jur_param_out_t;
int  jur_param_slices_host(jur_model_t *m, long nslice, long const *wptr, long const *bwptr,
                           long nr, int nd, long const *rowptr, long const *rowptr_b, int const *sid,
                           double const *gain, double const *kb, double const *weight_eff,
                           jur_param_in_t const *in, jur_param_out_t const *out);
long jur_param_layout(long nslice, long const *wptr, long nr, long const *rowptr, long const *rowptr_b, int const *sid,
                      long *bwptr, long *cptr, long *bbptr);
void jur_param_abi_sizes(size_t out[2]);   /* sizeof jur_param_in_t, jur_param_out_t: for bindings that mirror them */

/* Parameter errors of a scene in one call: jur_gain_scene_host, jur_kernel_scene_host under the parameters' windows and
 * jur_param_slices_host with the gain and K_b left on the device.  Every argument of jur_gain_scene_host as there, plus
 * jur_param_scene_in_t: ctl_b, of which the ret*_zmin/zmax windows define the parameters b and nothing else is read;
 *   rowptr_b [nr + 1], jur_scene_layout's for these rays and this atmosphere under those windows (JUR_EINVAL otherwise);
 *   in, laid out by jur_param_layout of (wptr, rowptr, rowptr_b, sid) as for jur_param_slices_host; bwptr [nslice + 1],
 *   that layout's, or NULL: where given it is checked against the widths.
 * jur_param_scene_out_t: out (C optional, sigma_param required when nvar + ncov > 0); kb optional, [rowptr_b[nr] * nd],
 *   the blocks of jur_kernel_scene_host under ctl_b; weight_eff optional, [nr][nd].
 * Contract: the doubles of the three calls, bit for bit.  rad, tau, tp, np_out, A, b, cost, nlive, k, every field of diag,
 *   gain and sigma_comp are jur_gain_scene_host's on the same arguments.  kb is jur_kernel_scene_host's k on a model whose
 *   windows are ctl_b's, with the same input mask.  weight_eff is the effective weight of jur_gain_scene_host (weight where
 *   the measurement is live -- with a field of view under the effective mask --, +0.0 elsewhere).  C and sigma_param are
 *   jur_param_slices_host's on those arrays.  Nothing depends on max_rays_per_pass, on which optional outputs were asked
 *   for or on the other slices.  A field of view, the hydrostatic balance per slice and a full prior precision of the
 *   model are honoured as the three entries honour them: the same code runs.
 *   One corner.  jur_param_slices_host pads the measurements of a slice to a multiple of 16 with exact zeros, and
 *   fma(+0, +0, c) turns a chain that stands at -0.0 into +0.0.  Here the chains of C are cut where the passes are, and each
 *   stretch is padded: an element of C can differ from jur_param_slices_host's in the sign of a zero, and only where a
 *   partial chain is exactly -0.0 at a pass boundary or at the end -- which takes products G * K_b that underflow to zero.
 * On the device.  Phase 1 is the body of jur_gain_scene_host; the gain and the effective weights are written to a buffer
 *   the model owns beside the slab of the scene entries.  Phase 2 runs the Jacobian passes under ctl_b's windows, cut by
 *   jur_scene_passes (rowptr_b, the cap; with a field of view whole scans); after the quotients of a pass the chains of C
 *   are continued over the live measurements of its rays, in accumulators that stay in that buffer; the blocks of a pass
 *   go home only where kb is given.  Phase 3 is the quadratic forms on the finished C.  No K_b beyond one pass is ever
 *   resident; the gain is copied home only where gout->gain is given.  The buffer (gain, weights, C, the parameter
 *   covariances, sigma_param, the layout) is counted against the workspace budget before everything else: JUR_ENOMEM
 *   before anything is launched where it does not fit in half of it, and max_rays_per_pass == 0 is derived from what is
 *   left.  jur_model_scene_bytes: the device bytes the scene entries hold at present, the slab and this buffer.
 * Refusals: what the three entries refuse, in their words under this entry's name.  Before anything is launched: the
 *   checks of jur_param_slices_host on nvar, ncov, var and cov, bwptr against the widths, rowptr and rowptr_b against the
 *   layouts, a NaN window in ctl_b.
 * The model's own retrieval windows are in force afterwards, after an error too, and it holds atm.  The kernels' time
 *   counts into jur_model_last_scene_ms. */
typedef struct {
  ctl_t const *ctl_b;
  long const *rowptr_b;        /* [nr + 1] */
  long const *bwptr;           /* [nslice + 1] or NULL */
  jur_param_in_t const *in;
} jur_param_scene_in_t;
typedef struct {
  jur_param_out_t const *out;
  double *kb;                  /* optional, [rowptr_b[nr] * nd] */
  double *weight_eff;          /* optional, [nr][nd] */
} jur_param_scene_out_t;
int  jur_param_scene_host(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double *rad, double *tau,
                          double *const tp[3], int *np_out, long const *rowptr, double const *y, double const *weight,
                          double const *prior_ivar, jur_diag_out_t const *diag, jur_gain_in_t const *gin, jur_gain_out_t const *gout,
                          jur_param_scene_in_t const *pin, jur_param_scene_out_t const *pout,
                          double *A, double *b, double *cost, long *nlive, double *k, long max_rays_per_pass);
void jur_param_scene_abi_sizes(size_t out[2]);   /* sizeof jur_param_scene_in_t, jur_param_scene_out_t */
long jur_model_scene_bytes(jur_model_t const *m);
/* the share of the per-pass kernel of phase 2 within jur_model_last_scene_ms (after jur_model_last_kernel_ms, as that) */
int  jur_model_last_cross_ms(jur_model_t *m, double *out_ms, long *out_launches);

/* The retrieval windows of a model.  A model keeps a copy of the control block it was created with, and every entry that
 * derives its state from it -- the scene entries (jur_kernel_scene_host ... jur_gain_scene_host) and jur_kernel, with
 * jur_state_size -- reads the windows there.  jur_model_set_ret_windows copies retp_zmin/zmax, rett_zmin/zmax,
 * retq_zmin/zmax[ng] and retk_zmin/zmax[nw], and nothing else, from ctl into that copy: from the next call on those
 * entries see the new windows, so one model (one upload of the tables) serves the Jacobian K and the Jacobian K_b of
 * quantities that are not retrieved.  No device work; nothing the model caches depends on the windows.  A prior
 * precision that is set (jur_model_set_prior_precision) is still checked against the layout of each call, as before.
 * JUR_EINVAL for a NULL or a window bound that is NaN; after a refusal what was set stays set.
 * jur_model_ret_windows copies the same fields out into ctl and leaves the rest of it alone. */
int  jur_model_set_ret_windows(jur_model_t *m, ctl_t const *ctl);
int  jur_model_ret_windows(jur_model_t const *m, ctl_t *ctl);

/* Curtis-Godson means along each line of sight (reference curtis_godson(), jr_common.h:455-473, which
 * upstream compiles only with -DCURTIS_GODSON for FORMOD=1): per ray, emitter and LOS point the
 * column-weighted pressure cgp, temperature cgt and the cumulative column cgu.  Host arrays
 * [nr][ng][JUR_NLOS]; entries from np[ray] on are 0.  tp (optional) and np_out (optional) as above. */
int  jur_curtis_godson_host(jur_model_t *m, long nr, double const *const geom[7],
                            double *cgp, double *cgt, double *cgu, double *const tp[3], int *np_out);

/* Field-of-view convolution on flat arrays (the arithmetic of formod_fov): time[nr], vpz[nr], rad/tau rows of
 * nd values with row stride ld, n weights w at altitude offsets dz (jur_fov_read_shape reads the
 * two-column file ctl->fov names, at most JUR_NSHAPE rows).  In place; host code. */
int  jur_fov_read_shape(char const *filename, int *n, double *dz, double *w);
int  jur_fov_apply(int nd, long nr, double const *time, double const *vpz, double *rad, double *tau, long ld,
                   int n, double const *dz, double const *w);

/* The same convolution for results that stay in HBM (after jur_formod_device): d_time / d_vpz [nr] and
 * d_rad / d_tau [nr][nd] in device memory of the model's GPU, convolved in place by a HIP kernel (one lane per
 * ray and channel, the arithmetic of formod_fov in its order: bit-identical to jur_fov_apply); dz / w are host
 * arrays.  Returns after the work on `stream` has finished; JUR_EINVAL if a ray is alone in its scan. */
int  jur_fov_apply_device(jur_model_t *m, long nr, double const *d_time, double const *d_vpz, double *d_rad,
                          double *d_tau, int n, double const *dz, double const *w, void *stream);

/* The field of view inside the scene entries.  A limb sounder's radiance is the forward model of a tangent-height scan
 * convolved with the instrument's field of view; with a shape set in the model the six scene entries --
 * jur_kernel_scene_host, jur_normal_scene_host, jur_step_scene_host, jur_trial_scene_host, jur_retrieve_scene_host and
 * jur_diagnose_scene_host -- apply that convolution on the device between the forward model and everything that reads
 * its radiances.  Nothing else honours the shape: jur_formod_*, jur_kernel, kernel(), the contribution entries and the
 * drop-ins compute pencil beams as before, and their caller applies jur_fov_apply / jur_fov_apply_device.
 *
 * jur_model_set_fov: n weights w at altitude offsets dz (what jur_fov_read_shape reads from the file ctl->fov names),
 *   kept on host and device; n == 0 switches the convolution off (the default: the scene entries then compute the bits
 *   and launch the kernels they did before).  JUR_EINVAL, naming the entry: n outside 0..JUR_NSHAPE; a dz or w that is
 *   not finite; weights whose sum in ascending order is 0 or not finite.
 * jur_model_fov: what is set; dz and w (room for JUR_NSHAPE each) may be NULL.
 * jur_scene_fov_live (host arithmetic, no GPU): the rule the device follows.  A scan is a maximal run of consecutive rays
 *   of the call with equal time stamps; the window of ray ir is the rays ir2 of [ir - JUR_NFOV, ir + JUR_NFOV] with
 *   time[ir2] == time[ir] (formod_fov's window).  JUR_EINVAL, naming the ray: a time stamp that occurs in two separate
 *   runs (the windows would change when the retrieval loop drops finished slices); a window of fewer than two rays
 *   (upstream's "Cannot apply FOV convolution!").  Otherwise live[ir][id] ([nr][nd], may be NULL) is 1 exactly when
 *   rad_in is finite in channel id on every ray of ir's window -- the effective mask, a superset of the channels where
 *   the convolution can touch a NaN, and a function of the inputs alone -- and the number of live entries is returned.
 * The scene entries while a shape is set:
 *   rad and tau out are the doubles of jur_formod_host followed by jur_fov_apply(nd, nr, geom[0], geom[4], rad, tau, nd,
 *   n, dz, w) on the call's rays in the caller's order (the input NaN mask applies to the pencil beams first; a NaN
 *   spreads where jur_fov_apply spreads it); tp and np_out are unchanged.  Block entry (id, e) is (G1 - G0) / h with G0
 *   that convolved radiance and G1 the same convolution of the forward model with element e raised: the quotient of
 *   convolved radiances, as kernel() differences formod's output, with layout, rowptr and columns unchanged.  In the
 *   sums and the costs F is G and "channel not masked on input" is the effective mask (a live measurement has a finite G;
 *   a trial G that is not finite makes that one cost NaN).  A scan is never split between passes: a pass is extended to
 *   the end of its scan, a scan beyond the cap goes alone, and no output depends on max_rays_per_pass.  What
 *   jur_scene_fov_live refuses is JUR_EINVAL before anything is launched; the model holds atm (atm0) afterwards.  The
 *   workspace accounting (JUR_ENOMEM) and the slots of a pass include the convolution's buffers.  The convolution kernel's
 *   time counts into jur_model_last_scene_ms. */
int  jur_model_set_fov(jur_model_t *m, int n, double const *dz, double const *w);
int  jur_model_fov(jur_model_t const *m, int *n, double *dz, double *w);
long jur_scene_fov_live(int nd, long nr, double const *time, double const *rad_in, unsigned char *live /* [nr][nd] or NULL */);

/* The passes of the scene entries (host arithmetic, no GPU): the rules the entries follow when max_rays_per_pass (cap
 * here, >= 1) or the workspace budget splits a call.  rowptr is jur_scene_layout's; time is the rays' time stamps while
 * a field of view is set and NULL otherwise.  JUR_EINVAL for bad arguments.
 * jur_scene_passes: the Jacobian entries.  A ray of width w takes w + 1 slots (itself and one copy per state element)
 *   and w block columns.  A pass is a contiguous range of rays, extended while its slots stay within cap; one ray beyond
 *   the cap goes alone; with time a pass is then extended to the end of its last scan.  pass (room for nr + 1 entries, or
 *   NULL) receives the first ray of every pass and nr; *nmax and *kmax (either may be NULL) the slots and the block
 *   columns of the largest pass.  Returns the number of passes, JUR_EINVAL (-1) for a pass of 2^31 slots.
 * jur_trial_passes: the trial passes, ntrial slots per ray: max(cap / ntrial, 1) rays each, with time extended to the end
 *   of the last scan.  Outputs and return value as above.
 * jur_scene_pass_reserve: what jur_retrieve_scene_host allocates.  Its loop gathers the rays of the slices that are
 *   still active and cuts both kinds of passes anew, and the cut of a subset can hold more than any pass of the first cut:
 *   *slots and *cols are bounds for every pass of either kind on any subset of the rays that ended slices can leave, the
 *   first cut among them.  Without time: slots = max(min(cap, all slots), widest ray + 1, trial slots of the first cut),
 *   cols = max(min(cap - 1, all columns), widest ray).  With time: the cap and one more scan, never more than the whole
 *   call.  With a cap under which the call is one pass of either kind they are the sizes of those passes. */
long jur_scene_passes(long nr, long const *rowptr, long cap, double const *time, long *pass, long *nmax, long *kmax);
long jur_trial_passes(long nr, int ntrial, long cap, double const *time, long *pass, long *nmax);
int  jur_scene_pass_reserve(long nr, long const *rowptr, long cap, int ntrial, double const *time, long *slots, long *cols);

/* A correlated a-priori covariance: the full prior precision of the slices.  The model holds, as it holds the field of
 * view, one symmetric matrix R_s per slice; while one is set the prior of the entries that take one --
 * jur_solve_slices_host, jur_step_scene_host, jur_trial_scene_host, jur_retrieve_scene_host, jur_diagnose_slices_host and
 * jur_diagnose_scene_host -- is P_s = R_s + diag(prior_ivar_s) in place of diag(prior_ivar_s).  Their prior_ivar (it may
 * be all zeros) and prior_dx / prior_xa are then required.  jur_kernel_scene_host and jur_normal_scene_host take no prior
 * and are unaffected.  With r = prior_ivar, d = prior_dx, every line reducing to the text of those entries when R = 0:
 *   D_i = A_ii + P_ii, P_ii = R_ii + r_i;  element i is live when D_i > 0.  The row and column of a dead element in A and
 *     in P are ignored; its dx, its rows and columns of S and AVK and its sigmas are +0.0.
 *   M = A + P + lam Z on the live elements, Z = diag(D) (JUR_DAMP_MARQUARDT: M_ii = fma(lam, D_i, D_i)) or Z = P
 *     (JUR_DAMP_PRIOR, the damping (1 + lam) Sa^-1 with its off-diagonals: M_ij = fma(lam, P_ij, A_ij + P_ij)).
 *   g_i = fma(r_i, d_i, b_i) + sum_j R_ij d_j over the live j;  M = L L^T, dx the solution;  pred = dx^T (g + lam Z dx):
 *     the solve's sum with Z = diag(D), and sum_i dx_i fma(lam r_i, dx_i, g_i) + lam (dx^T R dx) with Z = P.  Breakdown
 *     as there: status 1 + column, that system's outputs all zeros.
 *   jur_trial_scene_host: prior[t][s] = d^T P d, d = xa - (x + dx[t]), over all elements of the slice: the chain of the
 *     diagonal prior plus d^T R d.  jur_retrieve_scene_host: J = cost + prior with that prior; prior_dx = xa - x is formed
 *     on the device as before.
 *   Diagnostics: M = A + P (lam = 0), S = M^-1, AVK = S A (still the product), sigma_smooth_i = sqrt(max((S P S)_ii, 0))
 *     from the product S P; the rest as there.
 *   Every sum over a row of R takes lane l of 64 over j = l, l + 64, ... ascending as a chain of fused multiply-adds and
 *     then a fixed tree over the lanes; a quadratic form takes the rows i = k, k + 4, ... in four chains q_k = fma(v_i,
 *     (R v)_i, q_k) and returns (q_0 + q_1) + (q_2 + q_3).  Every double of a system depends on that system's inputs and
 *     on w alone: not on the batch, the order, nlam, max_rays_per_pass or the entry called.  No atomics.
 * jur_model_set_prior_precision: R_s at R + aptr[s], [w_s][w_s], aptr the running sum of w_s^2 with w_s = wptr[s + 1] -
 *   wptr[s]; symmetric, only its diagonal and lower triangle are read.  nslice == 0 or R == NULL: off (the default: every
 *   entry then launches what it launched before).  R is copied to device memory of the model's GPU here (JUR_ENOMEM,
 *   JUR_EHIP); after a refusal what was set before stays set.  Positive definiteness is not checked: a pivot that is not
 *   > 0 is the solve's breakdown status.
 * jur_model_prior_precision: returns nslice of what is set (0: off) and copies wptr and R where given.
 * JUR_EINVAL, naming the slice or the element, before anything is launched: an entry of R that is read and not finite; an
 *   R_ii < 0; wptr not ascending (set call); a call whose layout (nslice, widths) is not the one set, both counts named; a
 *   prior-taking entry called without prior_ivar while R is set.  The scratch the full prior adds (the assembled matrices
 *   and g; S P for the diagnostics; the differences of the trials) is part of each entry's JUR_ENOMEM accounting.
 * jur_prior_corr_host: the upstream parametrisation, built and inverted on the device.  Per slice, with iq and the point
 *   of every element from jur_scene_elements and z = atm->z[ip]:
 *     Sa_ij = (sigma_i sigma_j) exp(-(|z_i - z_j| / cz[q])) for iq_i == iq_j == q and cz[q] > 0;  Sa_ii = sigma_i^2;  0
 *     otherwise.  R_s = Sa_s^-1 by the solve's factorisation and the diagnostics' inverse: full, its two triangles
 *     bit-identical; status[s] is the solve's breakdown status (two elements of one quantity at one altitude make Sa
 *     singular: a breakdown where the rounded pivot is not > 0), R_s all +0.0 then.  Sa is optional.  JUR_EINVAL for a sigma
 *     that is not > 0 or not finite, a cz that is negative or not finite, an iq outside 0..nq-1, a z that is not finite.
 *   Correlation across slices is not modelled: slices are independent systems in this layer. */
int  jur_model_set_prior_precision(jur_model_t *m, long nslice, long const *wptr, double const *R);
long jur_model_prior_precision(jur_model_t const *m, long *wptr /* [nslice + 1] or NULL */, double *R /* or NULL */);
int  jur_prior_corr_host(jur_model_t *m, long nslice, long const *wptr,
                         int const *iq, double const *z, double const *sigma,   /* [wptr[nslice]] each */
                         int nq, double const *cz,                              /* [nq] correlation length per quantity, 0: uncorrelated */
                         double *R, double *Sa /* optional */, int *status /* [nslice] */);

/* Hydrostatic balance per slice in the scene entries.  ctl->hydz >= 0 makes formod() balance all points of the atmosphere
 * as ONE profile (hydrostatic_1d_h2o over 0..np), which couples every profile of a scene: the six scene entries refuse it,
 * now as before.  A retrieval of a scene wants upstream's other routine, hydrostatic() (jurassic.c:263-276), which balances
 * every profile on its own: a raised T element then moves the pressures of its own slice only, and the blocks, the sums
 * per slice, the independent systems and the trial passes keep their structure.  The model holds the switch as it holds
 * the field of view; off (the default) every entry launches what it launched before and returns the same bits.
 *
 * jur_scene_hydrostatic (host arithmetic, no GPU): the rule.  For every segment [sfirst[q], sfirst[q] + slen[q]) of two
 *   points or more, hydrostatic_1d_h2o (jr_common.h:713-761) on those points in the reference's order: the reference
 *   parcel ipref is the first point of the segment with the smallest |z - hydz| (strict <: a tie goes to the lower index),
 *   lat is lat[ipref], every layer takes the 20-term mean (i ascending) and p[to] = p[from] * exp(-1000 * mean * (z[to] -
 *   z[from])), the points above ipref upwards in index, then the points below downwards.  e is the H2O mixing ratio of
 *   the emitter jur_model_set_atm's step reads: the one named "H2O" when ctl->ctm_h2o is set, otherwise e = 0.  Only
 *   out->p is written (out may be in); p[ipref] keeps its value, so a second balance returns the same bits.  Segments of
 *   fewer than two points are left alone.  JUR_EINVAL, naming what is wrong: hydz negative or not finite; a segment
 *   outside 0..np; two segments of two points or more that share a point (both are named).
 * jur_scene_ray_slices (host arithmetic, no GPU): the distinct slices (first, len >= 2) that rays with the time stamps
 *   time[nr] are traced through, in the order the rays first meet them, whether or not they hold state elements (a ray
 *   of width 0 is traced through the base atmosphere and sees balanced pressures too); outputs may be NULL, room for nr
 *   entries each.  Returns their number.  This is the list the entries and jur_scene_hydrostatic_host balance.
 * jur_model_set_scene_hydz: the reference altitude [km]; a negative value switches the balance off (the default), NaN
 *   or infinity is JUR_EINVAL.  jur_model_scene_hydz: what is set (-1: off).  An atmosphere that jur_model_set_atm
 *   uploaded under one setting is not taken for current under another.
 * jur_scene_hydrostatic_host: atm_out = atm_in with p replaced by the balanced pressures on the ray slices of the rays
 *   with time stamps time[nr], formed by the one device kernel every entry launches (jur_scene_hydro_kernel: a wavefront
 *   per segment, the parcel from a fixed reduction over (|z - hydz|, index), the layers' factors dealt out over the lanes,
 *   the two chains sequential products in the reference's order; no atomics, every double a function of its own segment's
 *   inputs alone).  atm_out may be atm_in.  JUR_EINVAL when the switch is off; otherwise jur_scene_hydrostatic's
 *   refusals.  The model's atmosphere and workspace are untouched; the call is ordered against the model's other calls as
 *   jur_solve_slices_host is.  Against the host rule the pressures differ by the two exp and sin implementations alone
 *   (below 1e-12 relative over 150 levels; DESIGN.md has the measured figure).
 * The six scene entries while the switch is on, B(a) standing for jur_scene_hydrostatic_host(m, a, nr, geom[0], .):
 *   Overlapping ray slices are JUR_EINVAL before anything is launched; the model holds atm (atm0) afterwards.  The base
 *   rows on the device are balanced once over the ray slices before the first pass; the caller's atm is never written.
 *   rad, tau, tp and np_out are the doubles of jur_formod_host on B(atm) (a field of view, if set, applied afterwards as
 *   above).  After the stacking, the copies whose raised row is p, T or the H2O row are balanced again; the step h of a
 *   copy is the usual rule on the balanced base value.  Block entry (id, e) is (y1 - y0) / h with y1 the forward model on
 *   B(B(atm) with element e raised by h).  A p element that is not the reference parcel of its slice is overwritten by
 *   the balance: its block column is exactly +0.0 and the element is dead under the solve's D_i > 0 rule unless a prior
 *   holds it (upstream's kernel() behaves the same way): the sensible retrieval window for p holds the reference level
 *   only.  The sums, costs, steps and diagnostics follow from these blocks as their text says.  Trial copies are balanced
 *   after the elements have moved and before the trial rays: cost[t][s] is jur_normal_scene_host's cost on the atmosphere
 *   with dx[t] written back, the switch on.  In jur_retrieve_scene_host the base segments are balanced again after the
 *   accepted steps have been added; prior_dx = xa - x and x read the base rows as they then stand.  atm_ret is atm0 with
 *   the retrieved elements replaced and p replaced by the balanced pressure at every point of a ray slice (slices that
 *   ended early included; points in no ray slice untouched), so "rad is jur_formod_host on atm_ret" stays true without a
 *   balance in the forward entries; the model holds atm_ret afterwards, and atm as given after every other entry.
 *   Nothing depends on max_rays_per_pass; the field of view and the full prior precision work unchanged beside the
 *   balance.  The segment lists enter every entry's JUR_ENOMEM accounting, the kernel's time jur_model_last_scene_ms. */
int    jur_scene_hydrostatic(ctl_t const *ctl, double hydz, atm_t const *in, long nseg, int const *sfirst, int const *slen, atm_t *out);
long   jur_scene_ray_slices(ctl_t const *ctl, atm_t const *atm, long nr, double const *time, int *sfirst, int *slen);
int    jur_model_set_scene_hydz(jur_model_t *m, double hydz);
double jur_model_scene_hydz(jur_model_t const *m);
int    jur_scene_hydrostatic_host(jur_model_t *m, atm_t const *atm_in, long nr, double const *time, atm_t *atm_out);

/* A box on the state of the scene retrieval.  After every update of the state, before the forward model runs on it,
 * upstream's retrieval forces the atmosphere back into its physical range: p = min(max(p, 5e-7), 5e4), T = min(max(T, 100),
 * 400), q = min(max(q, 0), 1), k = max(k, 0).  Here the model holds one interval per quantity, off by default, and the two
 * entries that move a state honour it; with the box off every entry allocates, copies and launches what it did before and
 * returns the same bits.
 *
 * jur_state_bound: the rule, one text for host and device:  c = x > lo ? x : lo;  c = c < hi ? c : hi.  A NaN x gives lo
 *   (as upstream's GSL_MAX / GSL_MIN do); lo = -inf or hi = +inf leaves that side open.  Only state elements are bounded
 *   (the points inside the ret*_zmin/zmax windows, in jur_scene_elements' order); nothing else in the atmosphere is
 *   touched.  A first guess outside the box is not moved by itself: it enters the box with the first trial and the first
 *   accepted step.
 * jur_model_set_state_bounds: lo[nq], hi[nq] for the nq = 2 + ng + nw quantities in the iq numbering of
 *   jur_scene_elements (0 p, 1 T, 2 + g q, 2 + ng + w k).  nq == 0 or a NULL pointer switches the box off.  JUR_EINVAL,
 *   naming the quantity, for an nq that is not the model's, a NaN, or lo > hi (lo == hi holds the quantity fixed); after a
 *   refusal whatever was set before stays set.
 * jur_model_state_bounds: what is set into lo and hi (either may be NULL); returns nq, 0 when off.
 * jur_state_bounds_upstream (host arithmetic, no GPU): upstream's box above for the control's quantities (k: [0, +inf]);
 *   outputs may be NULL; returns nq.
 * jur_state_on_bounds (host arithmetic, no GPU): side[e] = -1 / 0 / +1 for an element x[e] of quantity iq[e] that equals
 *   its lower bound, neither bound, or its upper bound (lo == hi and x equal to both: -1); side may be NULL.  Returns the
 *   number of non-zero entries; JUR_EINVAL for an iq outside 0..nq-1.  This is how a caller finds the elements of out->x
 *   that the box holds: the diagnostics describe the unconstrained problem and do not know about the box.
 * jur_trial_scene_host while a box is set: the trial state of element e under trial t is bound(x_e + dx[t][e]) in every
 *   place the state is formed -- the stacked copy that is traced, the diagonal prior term, and the difference xa - state
 *   that the quadratic form of a full prior precision reads.  The contract keeps its form: cost[t][s] is, bit for bit, what
 *   jur_normal_scene_host returns on the atmosphere with the bounded step written back, prior[t][s] the documented chain
 *   on the bounded state.
 * jur_retrieve_scene_host while a box is set: the trial pass as above; an accepted slice moves to bound(x + dx[best]) in
 *   the base rows, so the next iteration's prior_dx = xa - x, the reuse iterations of jur_model_set_kernel_recomp, out->x,
 *   atm_ret and the final forward model all see the bounded state.  With jur_model_set_scene_hydz on the order is
 *   upstream's: bound first, then the balance, for trial copies and accepted base rows alike.  pred and the steps dx of
 *   the solver stay unbounded, and jur_retrieve_decide is unchanged.  A trial whose rays still leave the traceable range
 *   ends the call with JUR_ENLOS as before.
 * The box is expanded on the host into two arrays per element when a call starts, uploaded once, and counted in the
 *   entry's JUR_ENOMEM accounting before anything is launched; no launch is added (jur_scene_elements_kernel,
 *   jur_scene_prior_kernel and jur_scene_prior_diff_kernel apply the rule where they form x + dx).
 * Every other entry (jur_step_scene_host, jur_gradient_scene_host, jur_normal_scene_host, jur_kernel_scene_host, the
 *   diagnostics, jur_kernel) moves no state and ignores the setting. */
int    jur_model_set_state_bounds(jur_model_t *m, int nq, double const *lo, double const *hi);
int    jur_model_state_bounds(jur_model_t const *m, double *lo, double *hi);
int    jur_state_bounds_upstream(ctl_t const *ctl, double *lo, double *hi);
double jur_state_bound(double x, double lo, double hi);
long   jur_state_on_bounds(int nq, double const *lo, double const *hi, long n, int const *iq, double const *x, signed char *side);

/* The scene Jacobian reused between the iterations of a retrieval (upstream's KERNEL_RECOMP).  The model holds the switch
 * as it holds the field of view; with every == 1 (the default) jur_retrieve_scene_host allocates and launches what it did
 * before and returns the same bits.  Only jur_retrieve_scene_host honours it.
 *
 * jur_model_set_kernel_recomp: the Jacobian is recomputed every `every`-th iteration; every < 1 is JUR_EINVAL.
 *   jur_model_kernel_recomp: what is set.  Iteration `it` (0-based, the loop's own counter, one schedule for all slices) is a
 *   Jacobian iteration when it % every == 0 and a reuse iteration otherwise.
 * jur_gradient_scene_host: the gradient and the cost of a scene from blocks the caller holds.  geom, rad (read first for
 *   the NaN mask), tau, tp, np_out and rowptr as jur_normal_scene_host; k holds the blocks as jur_kernel_scene_host lays
 *   them out (block of ray r at k + rowptr[r] * nd, [nd][width]).  The forward model runs on atm for the nr rays alone, one
 *   slot per ray, every ray traced through the stacked base rows under the time stamp copy 0 of a Jacobian pass carries:
 *   rad, tau, tp and np_out are the doubles of jur_normal_scene_host on the same arguments, with a field of view set and
 *   with the hydrostatic balance on too.  Over the live measurements of slice s (jur_normal_scene_host's rule: the input
 *   radiance -- with a field of view the effective mask --, F and y finite, weight > 0), in ascending rays of the slice and
 *   within a ray in ascending channels, each from +0.0:
 *     d = y - F;  wd = weight * d;  b_s[i] = fma(K_r[id][i], wd, b_s[i]);  cost[s] = fma(wd, d, cost[s]);  nlive[s]++
 *   the chains of jur_normal_scene_host, so with k the blocks jur_kernel_scene_host returns on the same atm and rays, b, cost
 *   and nlive are jur_normal_scene_host's bit for bit.  One lane per state element (jur_scene_gradient_kernel), no atomics;
 *   the accumulators stay on the device across the passes, and nothing depends on max_rays_per_pass or on the other
 *   slices of the call.  Rows of k of measurements that are not live are never read (masked channels hold NaN there); the
 *   values of k are not checked, and a NaN in a live row reaches b of that slice only.  max_rays_per_pass caps the rays of
 *   a pass: the passes are jur_trial_passes(nr, 1, cap, ...), so a scan is never cut.  Refusals are those of
 *   jur_normal_scene_host, and k == NULL while the state has elements; JUR_ENOMEM before anything is launched when the
 *   blocks do not fit beside the stacked slices in half the workspace budget.  The model holds atm afterwards; the kernels'
 *   time counts into jur_model_last_scene_ms.
 * jur_retrieve_scene_host while every > 1: room for the blocks of all rays (rowptr[nr] * nd doubles) is reserved in the
 *   device slab (JUR_ENOMEM before anything is launched if they do not fit in half the budget), and a Jacobian iteration
 *   leaves its blocks -- with a field of view the convolved ones -- and its A there.  A reuse iteration zeroes b, cost and
 *   nlive only, runs forward-only passes (jur_trial_passes(n, 1, cap, ...)) over the rays of the slices that are still
 *   active, then the field of view, then jur_scene_gradient_kernel on the retained blocks, and goes on with the unchanged
 *   solve on the retained A (it factors a copy), the trial pass, the policy and the accepted steps.  h_work[2 it] of a
 *   reuse iteration is the number of rays traced for the gradient, the active rays; everything else is as with every == 1.
 *   A reuse iteration is jur_gradient_scene_host on the blocks of the active rays followed by jur_solve_slices_host on the
 *   A of the last Jacobian iteration, bit for bit.
 * jur_scene_recomp_offsets (host arithmetic, no GPU): where a reuse iteration finds the blocks.  A Jacobian iteration
 *   writes the blocks of the rays it traced -- the rays r with sid[r] >= 0 whose slice had then[sid[r]] == 0 (active) --
 *   back to back in ray order.  For the rays whose slice is active now (now[sid[r]] == 0), in ray order, koff receives the
 *   first double of each one's block: nd times the widths of the rays traced then that precede it.  Returns their number;
 *   JUR_EINVAL when a slice is active now that was not then. */
int  jur_model_set_kernel_recomp(jur_model_t *m, int every);
int  jur_model_kernel_recomp(jur_model_t const *m);
int  jur_gradient_scene_host(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double *rad, double *tau,
                             double *const tp[3], int *np_out, long const *rowptr, double const *y, double const *weight,
                             double const *k /* blocks, as jur_kernel_scene_host lays them out */,
                             double *b, double *cost, long *nlive, long max_rays_per_pass);
long jur_scene_recomp_offsets(long nr, long const *rowptr, int const *sid, int const *then, int const *now, int nd, long *koff);

/* Untraceable rays in the scene retrieval: a trial whose rays overflow is a rejected step, not an error.  The model holds
 * the switch as it holds the field of view; with JUR_OVERFLOW_ERROR (the default) every entry allocates and launches what
 * it did before and returns the same bits.  Only jur_trial_scene_host and jur_retrieve_scene_host honour it; the other
 * scene entries and jur_formod_* keep JUR_ENLOS.
 *
 * jur_model_set_scene_overflow: JUR_OVERFLOW_ERROR (a ray that needs JUR_NLOS points or more ends the call with
 *   JUR_ENLOS) or JUR_OVERFLOW_ISOLATE; any other mode is JUR_EINVAL.  jur_model_scene_overflow: what is set.
 * jur_np_overflows (host arithmetic, no GPU; one text with the device): np >= JUR_NLOS - 1.  The tracer clamps a ray that
 *   needs more to JUR_NLOS - 1 points and keeps no flag per ray, so a ray that fills the array counts as untraceable
 *   whether or not it was clamped: the rule errs towards rejection, and it depends on the ray alone -- not on the status
 *   word, which all rays of a call share.
 * With JUR_OVERFLOW_ISOLATE, on the device (jur_scene_overflow_kernel after the forward model of every pass, one fold
 *   per kind of pass; no atomics, no host wait of their own):
 *   Trial passes (jur_trial_scene_host, the trial pass of the loop): where a ray of (slice s, trial t) overflows,
 *     cost[t][s] is NaN; prior[t][s] and every other double of the call are bit for bit what they are without that
 *     trial's overflow, and the entry returns JUR_OK.  In the loop that trial's h_status is JUR_TRIAL_OVERFLOW and its
 *     h_tcost NaN; jur_retrieve_decide is unchanged (a NaN Jt is no candidate), so the step is rejected and lam grows.
 *     A ray without state elements belongs to no slice and poisons nothing.
 *   Jacobian, reuse and gradient passes of the loop: where a slot of a slice's rays overflows (copy 0 or a raised copy)
 *     the slice becomes JUR_RET_FAILED once all passes of the iteration are done and before its solve; the solve, the
 *     trial copies, the prior terms and the trial costs skip it as they skip every ended slice.  (The passes of that
 *     iteration have by then added the slice's rays, clamped ones included, to its own A, b, cost and nlive on the
 *     device: those sums are never read -- not by the solve, not by the host, not by another slice -- and the slice's
 *     rays are in no later pass.)  A reuse or gradient pass traces the current state alone, which the pass that accepted
 *     it has traced already with the same result, so in practice only a Jacobian pass flags a slice.  iters is not incremented, the history cells of that iteration read
 *     "took no part", x stays the last accepted state (the first guess at iteration 0), cost, prior and nlive are those
 *     of the last completed iteration (NaN, NaN and 0 at iteration 0), and its rays are in no later pass.  All other
 *     slices proceed, every output of theirs bit for bit that of the call without the failed slice's rays.
 *   The call returns JUR_OK and atm_ret is written as on success; rad, tau, tp and np_out are what jur_formod_host writes
 *     for atm_ret (for a ray with jur_np_overflows(np_out): before it returns JUR_ENLOS); the model holds atm_ret and the
 *     status word is clean for the next call.  "Cannot apply FOV convolution!" and every JUR_EHIP, JUR_EINVAL and
 *     JUR_ENOMEM path end the call as before.  The flags and the partial counts are part of the slab's JUR_ENOMEM
 *     accounting, made before anything is launched.
 * jur_model_last_scene_overflow: of the last jur_trial_scene_host or jur_retrieve_scene_host call, the (trial, slice)
 *   cells whose cost was made NaN (summed over the iterations of a loop) and the slices that ended JUR_RET_FAILED; both 0
 *   with JUR_OVERFLOW_ERROR.  Either output may be NULL. */
enum { JUR_OVERFLOW_ERROR = 0, JUR_OVERFLOW_ISOLATE = 1 };
enum { JUR_RET_FAILED = 4 };              /* joins JUR_RET_ACTIVE .. JUR_RET_MAXITER */
enum { JUR_TRIAL_OVERFLOW = -2 };         /* a value of h_status: -1 took no part, 0 solved, > 0 the solver's */
int  jur_model_set_scene_overflow(jur_model_t *m, int mode);
int  jur_model_scene_overflow(jur_model_t const *m);
int  jur_model_last_scene_overflow(jur_model_t const *m, long *trial_cells, long *failed_slices);
int  jur_np_overflows(int np);

/* intpol_atm with an error code instead of exit(): JUR_EINVAL for what upstream aborts on (profiles of one point,
 * profiles more than 10 degrees apart, unknown IP).  One lane per destination point on `device`. */
int  jur_intpol_atm(ctl_t const *ctl, atm_t *dest, atm_t const *src, int device);

/* Allocate the workspace for calls of up to nr rays now.  jur_formod_device allocates lazily on
 * first use; after jur_model_reserve (or one call of the same size) it only enqueues kernels on
 * the stream -- no allocation, no host synchronisation -- and can be captured into a HIP graph. */
int  jur_model_reserve(jur_model_t *m, long nr);

/* Bytes of device workspace the model holds for `nr` rays per call, and the
 * chunk size (rays per kernel launch) it uses. */
long jur_model_workspace_bytes(jur_model_t const *m);
int  jur_model_chunk_rays(jur_model_t const *m);
/* Bytes of device memory the model's tables hold (entries, bracket slopes, descriptors). */
long jur_model_table_bytes(jur_model_t const *m);
/* PCI bus id (text, e.g. "0000:0c:00.0"; len >= 16) and the free / total device memory of `device` right now: what a
 * multi-GPU caller records and plans its workspace budget with. */
int  jur_device_info(int device, char *pci_bus_id, int len, size_t *free_bytes, size_t *total_bytes);
/* Tuning knobs: rays per chunk; whether rays are processed in order of their
 * geometric tangent altitude (default on; results do not depend on it). */
int  jur_model_set_chunk_rays(jur_model_t *m, int rays);
int  jur_model_set_sort_rays(jur_model_t *m, int on);
/* Rays per ray-tracing launch as a multiple of the rays per integration launch (default 1). */
int  jur_model_set_trace_multiple(jur_model_t *m, int mult);
/* Calls whose rays do not fit the workspace at JUR_NLOS points per ray (several integration launches) lay the
 * transmittance tiles out by the path lengths that occur (default on): all rays are traced first, the longest path of
 * every tile of 64 sorted rays comes back to the host -- ONE wait inside such a call; calls that fit in one launch, and
 * calls being captured into a graph, never wait -- and consecutive tiles are packed into launches of equal size.
 * Nadir rays use 182 of the 400 points: 2.2 x the rays per launch.  Same results bit for bit.
 * jur_model_last_launches: integration launches (jur_ega_kernel / jur_combine_kernel pairs) of the last batched call. */
int  jur_model_set_compact_workspace(jur_model_t *m, int on);
long jur_model_last_launches(jur_model_t const *m);
/* Upper bound of the per-call device workspace (LOS state + per-segment gas
 * transmittances); the rays-per-chunk shrink to fit.  Default 128 GiB of the 288 GB. */
int  jur_model_set_workspace_budget(jur_model_t *m, long bytes);

/* Calls of up to max_rays rays (default 10000; 0: never) run as ONE fused kernel -- ray tracing, emissivity growth
 * and radiance update of a ray as producer/consumer wavefronts of one workgroup, the line of sight handed on through
 * LDS -- instead of the three batched kernels: the sizes the reference's callers use (packages of <= NR rays).
 * rays_per_group: rays per workgroup, 0 = chosen from the call size.  Configurations with more (channel, gas)
 * chains per ray than the LDS rings hold use the batched kernels whatever the size.  Same results bit for bit.
 * The fused kernel is emissivity growth only: a model whose control block says FORMOD 1 accepts the call and runs
 * every size through the batched kernels (jur_model_last_pencil_ms reports no launch). */
int  jur_model_set_pencil(jur_model_t *m, long max_rays, int rays_per_group);
/* Process-wide: lanes per ray of the batched ray tracer (1 or 4; 0 = chosen per launch: a quad of lanes per ray for
 * launches of up to 65 536 rays with at least three emitters, one lane otherwise).  With four lanes the refraction
 * probes of a step (jr_common.h:665-681) and the emitters' columns are taken side by side; same results bit for bit
 * (tests/test_multi_gpu.py). */
void jur_tune_trace(int lanes_per_ray);
/* Process-wide: whether one-lane-per-ray launches of the batched ray tracer keep the profile slice of a workgroup's
 * rays in LDS (workgroups of 256 rays; rows z, p, T, ln-p slope, q[ng], k[nw], at most 1280 doubles for the longest
 * slice).  0 = chosen per launch (slice-sorted launches of at least 262 144 rays whose longest slice fits), 1 = never,
 * 2 = wherever the longest slice fits.  A workgroup whose rays use two slices reads the model's arrays.  Same results
 * bit for bit (tests/test_trace_lds_gpu.py). */
void jur_tune_trace_slice(int mode);
/* Process-wide: whether a batched call whose rays were sorted and fit ONE ray-tracing launch starts that launch's blocks
 * of 256 sorted slots in ascending order of the tangent altitude of their lowest ray, i.e. longest paths first, in the
 * one-lane-per-ray tracers and, where one integration launch covers the same slots, in the radiance update (instead of
 * in slot order, which ends every launch on the long blocks of the last profiles).  0 = chosen per call (at least
 * 262 144 rays), 1 = never, 2 = whenever the rays were sorted and the call is one trace launch.  Placement only: same
 * results bit for bit (tests/test_block_order_gpu.py). */
void jur_tune_block_order(int mode);
/* The block order of the model's last batched call, for tests and tools: copies up to `cap` entries to `out` (a
 * permutation of 0 .. n - 1) and returns n = (rays + 255) / 256, 0 if the call built none, JUR_EHIP on failure. */
long jur_model_block_order(jur_model_t *m, int *out, long cap);
/* Process-wide: whether the look-up kernel takes that block order too, where its launch covers the slots of the trace
 * launch (the nd * ng pair workgroups of a ray block still follow each other on one XCD).  1 = yes, 0 = the look-up in
 * slot order (default: the order was measured to leave the look-up's time where it is), < 0 = back to the environment's
 * JUR_BLOCK_ORDER_EGA.  Placement only: same results bit for bit (tests/test_ega_block_order_gpu.py). */
void jur_tune_block_order_ega(int mode);
/* Extinction of an atmosphere without any.  Where every extinction value of the atmosphere a caller has set is +0.0 and
 * the atmosphere is sorted (time stamps non-decreasing, z strictly monotone in every profile), the ray tracer neither
 * interpolates nor stores the nw extinction fields of a LOS point and the kernels that would read them take 0.0: the
 * value the interpolation of two zeros gives, so every result stays what it was bit for bit
 * (tests/test_extinction_elision_gpu.py).  jur_atm_k_zero is that decision for `count` extinction values `k` of rows
 * of the given origin: only JUR_ATM_CALLER rows qualify -- never the perturbed atmospheres of kernel() or of the
 * hydrostatic contribution variants, never rows stacked on the device (scene Jacobian, retrieval).
 * jur_model_k_zero: whether the model's next launch leaves the extinction out (0 without an atmosphere).
 * jur_tune_k_elision, process-wide: 1 = as above (default), 0 = never, < 0 = back to the environment's JUR_K_ELISION. */
enum { JUR_ATM_CALLER = 0, JUR_ATM_PERTURBED = 1, JUR_ATM_DEVICE = 2 };
int  jur_atm_k_zero(double const *k, long count, int atm_sorted, int origin);
int  jur_model_k_zero(jur_model_t *m);
void jur_tune_k_elision(int mode);
/* Process-wide tuning of the radiance-update kernel of the batched path: up to `channels_per_group` (0 .. 6, default
 * 4; 0 = one channel per workgroup always) channels of a ray block share a workgroup, with a barrier every
 * `sync_segments` segments (default 8; <= 0 none), for launches of at least `min_lanes` rays x channels (default
 * 1 000 000).  Without a call (or after one with channels_per_group < 0) the library groups by four, and only when
 * the channel count is a multiple of four: other group shapes were measured slower than one channel per workgroup.
 * Results do not depend on it (tests/test_parity_gpu.py compares the arrangements bit for bit). */
void jur_tune_combine(int channels_per_group, int sync_segments, long min_lanes);

/* Arithmetic of the emissivity-growth look-up, per model (process default: JUR_ARITH_FAST, or JUR_ARITH_EXACT when
 * the environment has JUR_EGA_NO_RCP set).
 *   JUR_ARITH_FAST   strictly increasing tables (every table that passes the reference's row rule) are interpolated
 *                    through bracket slopes formed once per model, blended through reciprocal bracket widths, and the
 *                    path transmittance is carried as 1 - eps: within ~1e-13 of the reference's divisions on
 *                    transmittances, ~6e-12 relative on radiances (the contract is 1e-6), a seventh fewer instructions;
 *   JUR_ARITH_EXACT  the reference's divisions operand for operand (jr_common.h:156-185, 237-268) -- what tables that
 *                    are not strictly increasing get in either mode.  For difference quotients with steps so small
 *                    that 1e-12 of a radiance matters (jur_kernel on mixing ratios that are zero: see there).
 * The fused kernel and the batched kernels follow the same switch, so they stay bit-identical to each other. */
enum { JUR_ARITH_FAST = 0, JUR_ARITH_EXACT = 1 };
int  jur_model_set_arithmetic(jur_model_t *m, int mode);
int  jur_model_arithmetic(jur_model_t const *m);

/* Band model, ctl->formod (FORMOD in a control file): 2 (default) the emissivity-growth approximation, 1 the
 * Curtis-Godson approximation (CGA).  Upstream computes the Curtis-Godson means and asserts FORMOD 1 out
 * (jr_common.h:701-707); here it runs, through every entry, with one rule.  For one ray, gas g, channel d, LOS points
 * ip = 0 .. np - 1 with p, T and the gas's column u (the records jur_kat_traceray shows):
 *   means   a += u p, b += u T, w += u from 0, products and sums rounded separately (no fma), in the order of
 *           curtis_godson() (jr_common.h:455-473); cgp = a / w, cgt = b / w, cgu = w by true divisions;
 *   path transmittance tau of the gas after segment ip, from tau_prev (1 before the first segment):
 *     1. tau_prev < 1e-9: 0 (the opaque gate of ega_eps, jr_common.h:239);
 *     2. no table for (g, d), or one of the nt < 2 / nu < 2 rules of ega_eps (:240-246) at (cgp, cgt): tau_prev;
 *     3. w == 0 (nothing of the gas on the path so far): tau_prev, tested before any bracket search;
 *     4. otherwise ipr = locate_id(p axis, cgp), it0 / it1 = locate_id(T axes of levels ipr, ipr + 1, cgt), the four
 *        corners e = c01(get_eps(curve, cgu)), two blends in T at cgt and one in p at cgp, each c01(lip(...)) as in
 *        ega_eps (:259-265): tau = 1 - eps_t.
 *   tau is not limited to tau_prev: a Curtis-Godson path transmittance may rise from one segment to the next.  The
 *   radiance update (segment transmittance of all gases as the quotient of the products of path transmittances,
 *   continua, source, surface, brightness temperature) is the one of FORMOD 2.
 * jur_model_set_arithmetic chooses between the reference's divisions and the strict-table arithmetic as for the
 * emissivity-growth look-up.  The look-up runs in the batched kernels only: the fused kernel of small calls does not
 * know the Curtis-Godson rule, so FORMOD 1 calls of any size take the ray sort and the three batched kernels
 * (jur_model_set_pencil stays accepted and has no effect).  Slot [1] of jur_model_last_kernel_ms counts whichever
 * look-up kernel ran. */

/* Atmosphere along the line of sight, ctl->ip (IP in a control file): 1 (default) one vertical profile per ray, chosen
 * by its time stamp; 2 a satellite track: every point of the line of sight is interpolated between the two nearest
 * profiles of a track (intpol_atm_2d, jurassic.c:704-760).  Upstream's GPU tracer asserts IP 1 (jr_common.h:573, 581);
 * here IP 2 runs in the ray tracer, with one rule, and IP 3 (a cloud of air parcels) with the rule further down.
 *   1. Time block.  A ray's time stamp selects the block [a0, a0 + n) of atmosphere points as under IP 1 (locate_atm);
 *      zmin .. zmax is the altitude range of the block's first column, as under IP 1.
 *   2. Profiles.  A profile is a maximal run of consecutive points with equal time stamp, longitude and latitude, so
 *      the profiles of a block are consecutive.  The table is built on the host with every atmosphere: first point,
 *      length and x1 = geo2cart(0, lon, lat) in the host's libm per profile, as upstream caches them.  An upload is
 *      refused with JUR_EINVAL and upstream's words when a profile has fewer than two points ("Cannot identify
 *      profiles. Check ordering of data points!") or two consecutive profiles of a block lie more than 10 degrees of
 *      latitude apart ("Distance of profiles is too large!"); the model holds no atmosphere afterwards.  A ray whose
 *      block is not made of whole profiles (its time stamp matches no run of equal time stamps) is not entered.
 *   3. Horizontal weights at a point (z, lon, lat), lon and lat from cart2geo of the position: x0 = geo2cart(0, lon,
 *      lat); among the block's profiles with |lat - lat_ix| <= 10, in table order, dh = DIST2(x0, x1[ix]);
 *      dh <= dhmin0 makes ix the nearest and the nearest the second, else dh <= dhmin1 makes it the second (both from
 *      1e99, ix0 = ix1 = the block's first profile).  x2 = DIST2(x1[ix0], x1[ix1]), x = sqrt(x2),
 *      r0 = (dhmin0 - dhmin1 + x2) / (2 x), r1 = x - r0; r = 0 if r0 <= 0, else 1 if r1 <= 0, else r0 / (r0 + r1):
 *      beyond the end of a track a point takes the end profile.
 *   4. Vertical interpolation, in either profile on its own levels at the bracket locate() finds there: p by eip,
 *      T, every q and every k by lip; then y = (1 - r) y0 + r y1, in that form.
 *   5. Every evaluation of the tracer takes 3 and 4: the LOS point (p, T, q, k, the columns u, q_H2O), the mid-step
 *      probe and the three displaced probes of the refractivity gradient, the columns redone for the point before the
 *      exit, and tsurf.
 *   A block with one profile gives ix0 = ix1, x = 0, r0 = -inf, r = 0 and y0 + 0 y1 = y0: the bits of IP 1 for finite
 *   profiles.  A point with no profile inside the 10-degree gate yields NaN by this arithmetic.
 * One kernel traces it (jur_track_trace_kernel, a lane per ray, all profiles of the block scanned at every evaluation);
 * the fused kernel of small calls stays 1-D, so IP 2 calls of any size take the batched kernels (jur_model_set_pencil
 * stays accepted and has no effect).  Forward model, contributions, Curtis-Godson columns, the dense Jacobian
 * (jur_kernel), the multi-device entries and the drop-in entries run under IP 2, with FORMOD 1 or 2.  The scene entries
 * (jur_kernel_scene_host and everything built on its per-ray blocks of ONE slice's state, the trial pass and the
 * retrieval loop included) return JUR_EINVAL before anything is launched: under IP 2 a ray reads two profiles.
 *
 * jur_track_profiles: the profile table of `atm` by rule 2, host only: first[], len[] (atmosphere points), x1[][3],
 * block_of[] (number of the profile's time block, from 0) hold one entry per profile -- room for atm->np / 2 + 1
 * entries each; any of them may be NULL.  Returns the number of profiles, or JUR_EINVAL with the words above. */
long jur_track_profiles(atm_t const *atm, int *first, int *len, double (*x1)[3], int *block_of);

/* ctl->ip == 3, a point cloud: every point of the line of sight is the distance-weighted mean over the air parcels
 * around it (intpol_atm_3d, jurassic.c:763-804), with ctl->cx and ctl->cz (CX, CZ in a control file) the horizontal and
 * vertical influence lengths in km.  jur_model_create refuses cx or cz that is not > 0 or not finite with JUR_EINVAL
 * (upstream would return NaN everywhere), and an ip other than 1, 2 or 3.  For one ray:
 *   1. Slice.  The ray's time stamp selects the atmosphere points [a0, a0 + n) exactly as under IP 1 and IP 2
 *      (locate_atm).  These points, and no others, are the cloud of that ray -- not upstream's literal loop over all
 *      atm->np points: the departure the IP 2 rule makes too.
 *   2. Altitude range.  zmin and zmax are the minimum and maximum of z over ALL points of the slice, by fmin / fmax in
 *      ascending index.  Upstream's first-column rule (altitude_range_nn, jr_common.h:411-420) is degenerate for a
 *      cloud, where no two points share a longitude and latitude; for a slice made of columns on one altitude grid
 *      the two agree.  The exclusions stay: zmin == zmax and a slice of fewer than two points are not entered.
 *   3. Cached positions.  x1[ip] = geo2cart(0, lon[ip], lat[ip]) for every atmosphere point, in the host's libm, once
 *      per upload: what upstream caches.
 *   4. Mean at a position.  The position gives z0; lon0, lat0 come from cart2geo of it and x0 = geo2cart(0, lon0,
 *      lat0).  With rm2 = cx * cx, over the slice's points in ascending index: skip the point if dz = |z[ip] - z0| >=
 *      cz; skip it if |lat[ip] - lat0| * 111.13 >= cx; dx2 = DIST2(x0, x1[ip]), skip it if dx2 >= rm2; otherwise
 *      w = (1 - dz / cz) * (rm2 - dx2) / (rm2 + dx2), wsum += w and y += w * y[ip] for p, T, every q and every k.
 *      Every product and sum is rounded on its own (no fused multiply-add); pressure is averaged linearly, as upstream
 *      does, not through eip.  Finally y /= wsum by a true division when wsum >= 1e-6, otherwise every value is NaN.
 *   5. Every evaluation of the tracer takes 4: the LOS point (p, T, q, k, the columns u = 10 q p / (k_B T) ds, q_H2O),
 *      the mid-step probe and the three displaced probes of the refractivity gradient, the columns redone for the
 *      point before the exit, and tsurf.
 *   6. Holes.  A position with no parcel inside its influence region yields NaN by this arithmetic.  With refraction
 *      off the NaN reaches that ray's records (p, T, q, k, u of the points in the hole), and those of no other ray;
 *      the radiance update then leaves out every segment whose gas transmittance is not > 1e-50, a NaN one included,
 *      exactly as upstream's new_obs_core does (jr_common.h:293-300), so the ray's radiance stays finite and misses
 *      those segments (tests/test_cloud_gpu.py holds it to the CPU model's, NaN for NaN and value for value).
 *      With refraction on the direction becomes NaN and the ray fills the LOS array: JUR_ENLOS.  The elision of an
 *      atmosphere without extinction is never taken under IP 3, so a hole gives NaN in k as well.
 * One kernel traces it (jur_cloud_trace_kernel, a lane per ray, the whole slice scanned at every evaluation; the
 * slice's z, lat and x1 staged in LDS where a workgroup's rays agree on a slice of at most jur_cloud_lds_points()
 * points: same doubles either way).  The fused kernel of small calls stays 1-D (jur_model_set_pencil stays accepted
 * and has no effect).  Forward model, contributions, Curtis-Godson columns, the dense Jacobian (jur_kernel), the
 * multi-device entries and the drop-in entries run under IP 3, with FORMOD 1 or 2, and ctl->hydz as under IP 2.  The
 * scene entries return JUR_EINVAL before anything is launched, as under IP 2.
 *
 * jur_cloud_points: rule 3 for `atm`, host only: x1 has room for atm->np entries.  Returns atm->np, or JUR_EINVAL.
 * jur_cloud_lds_points: the largest slice the tracer stages in LDS (a compiled constant). */
long jur_cloud_points(atm_t const *atm, double (*x1)[3]);
int  jur_cloud_lds_points(void);

/* Frees the process-global state behind formod() / formod_GPU() / formod_pencil(): the lanes (streams, atmosphere,
 * workspaces, pinned images) and the emissivity tables loaded by the first call.  Upstream keeps its counterparts for
 * the life of the process (GPUdrivers.cu:263-273, 309; jr_common.h:60-78).  Waits for calls in flight; returns the
 * number of lanes freed (0: nothing was initialised).  The next formod() loads the tables again. */
int  jur_dropin_finalize(void);

/* Summed duration in ms and launch count of each kernel since the last query,
 * measured with HIP events on the launch stream while timing is enabled:
 * [0] jur_trace_kernel, [1] jur_ega_kernel, [2] jur_combine_kernel. */
int  jur_model_enable_timing(jur_model_t *m, int on);
int  jur_model_last_kernel_ms(jur_model_t *m, double out_ms[3], long out_launches[3]);
/* ... and of the fused kernel (call jur_model_last_kernel_ms first) */
int  jur_model_last_pencil_ms(jur_model_t *m, double *out_ms, long *out_launches);
/* ... and of the contribution kernel (jur_contrib_kernel; call jur_model_last_kernel_ms first) */
int  jur_model_last_contrib_ms(jur_model_t *m, double *out_ms, long *out_launches);

/* ---- known-answer hooks (for tests; not on the product path) -------------------------------------------
 * The device functions of the path evaluated on host arrays of n inputs, one element per lane, so that each can be
 * checked against its reference counterpart at thresholds and range edges.
 * jur_kat_ega_eps: ega_eps (jr_common.h:237-268) of pair (ig, id).  mode 0 = the reference's bisections,
 *   1 = warm-started searches, 2 = + descriptors in LDS, 3 = + reciprocal bracket widths (what the bench runs);
 *   JUR_EINVAL when the tables do not admit the mode.  chain != 0: one lane evaluates the n inputs in order,
 *   carrying the search state from one to the next as the kernel does along a ray.
 * jur_kat_cga_eps: the Curtis-Godson look-up of pair (ig, id) (FORMOD 1, see there): out[i] = the new path transmittance
 *   by steps 1, 2 and 4 from tau[i] and the means cgt[i], cgu[i], cgp[i]; modes and chain as for jur_kat_ega_eps
 *   (0 = the reference's bisections and divisions, 3 = what jur_cga_kernel runs on strict tables).
 * jur_kat_continua: out[4][n] = continua_ctmco2/h2o/n2/o2 (jr_common.h:315-390) of channel id (0 outside a window).
 * jur_kat_update: what 0: src[i] = src_planck_core(a[i]); (rad, tau)[i] updated by new_obs_core with
 *   tau_gas = b[i], beta_ds = c[i] (jr_common.h:220-224, 293-300); what 1: add_surface_core with surface
 *   temperature a[i] and, if b[i] != 0, brightness_core (jr_common.h:187-190, 227-234).
 * jur_kat_traceray: the LOS records the batched ray tracer writes for nr rays (traceray, jr_common.h:585-711), through
 *   the launches jur_formod_host makes (rays per launch as jur_model_set_chunk_rays leaves them, lanes per ray as
 *   jur_tune_trace says).  geom, tp (optional), np_out (optional) as in jur_formod_host.  los is a host array
 *   [nr][nfield][JUR_NLOS], nfield = 4 + nw + ng, rows p, T, ds (trapezoid weight), q_H2O, k[nw], u[ng] (column
 *   densities); entries from np[ray] on are 0, and so is the q_H2O row when the model has no H2O continuum emitter
 *   (the tracer never writes it then).  tsurf [nr]: the surface temperature of a ray that hits the ground, else -999.
 *   JUR_ENLOS, with the records clamped to JUR_NLOS - 1 points, when a ray overflows.  The fused kernel hands its
 *   records on through LDS and cannot be read this way. */
int jur_kat_ega_eps(jur_model_t *m, int ig, int id, long n, double const *tau, double const *t, double const *u,
                    double const *p, int mode, int chain, double *out);
int jur_kat_cga_eps(jur_model_t *m, int ig, int id, long n, double const *tau, double const *cgt, double const *cgu,
                    double const *cgp, int mode, int chain, double *out);
int jur_kat_continua(jur_model_t *m, int id, long n, double const *p, double const *t, double const *q,
                     double const *u_co2, double const *u_h2o, double *out);
int jur_kat_update(jur_model_t *m, int id, long n, int what, double const *a, double const *b, double const *c,
                   double *rad, double *tau, double *src);
int jur_kat_traceray(jur_model_t *m, long nr, double const *const geom[7], double *los, double *tsurf, double *const tp[3],
                     int *np_out);
/* jur_kat_cloud_mean: rule 4 of IP 3 (the model must have been created with ip = 3 and hold an atmosphere) on the
 * device at n positions given AFTER the geometry step -- z0[i], lat0[i] and x0[i] = geo2cart(0, lon0, lat0) -- over the
 * atmosphere points [a0, a0 + len), one position per lane: out [2 + ng + nw][n] holds p, T, every q, every k.  The
 * device's sin and cos play no part, so the result is comparable bit for bit.  Slices of up to
 * jur_cloud_lds_points() points are read from LDS as the tracer reads them, longer ones from the model's arrays. */
int jur_kat_cloud_mean(jur_model_t *m, long n, int a0, int len, double const *z0, double const *lat0, double const (*x0)[3],
                       double *out);

#ifdef __cplusplus
}
#endif
#endif
