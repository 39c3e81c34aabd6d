/* jur_model.c -- host orchestration: device residency of a model, the batched
 * formod entry points and the drop-in formod()/formod_GPU()/formod_pencil().
 *
 * Plain C over the HIP runtime C API.  There is deliberately no CPU fallback:
 * without a GPU every entry point fails loudly.
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <pthread.h>
#include <unistd.h>
#include <sched.h>
#include <hip/hip_runtime_api.h>
#include "jur_internal.h"

#define HIPCHK(call)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess) {                                                                \
      jur_set_error("HIP error %d (%s) at %s:%d", (int)e_, hipGetErrorString(e_), __FILE__, __LINE__); \
      return JUR_EHIP;                                                                     \
    }                                                                                      \
  } while (0)

struct jur_model {
  int device;
  int shared_tables;            /* 1: a lane of the drop-in entry; the table arrays belong to another model */
  ctl_t *ctl;                   /* private copy of the control block             */
  jur_view_t view;              /* device pointers                               */
  long table_bytes;
  /* device allocations owned by the model */
  void *d_chan, *d_sr, *d_pair, *d_pair_e0, *d_lvl, *d_crv, *d_ue, *d_rec;
  int arith;                    /* JUR_ARITH_*                                   */
  void *d_atm;                  /* one slab for the compact atmosphere           */
  jur_track_t track;            /* ctl->ip and, under ip == 2, the profile table of the atmosphere on the device */
  void *d_track;                /* its grow-only slab: x1 | lat as doubles, then first | len | dir | prof_of as ints */
  size_t track_bytes;
  jur_cloud_t cloud;            /* under ip == 3: cx, cz and the cached position of every point of the atmosphere on the device */
  void *d_cloud;                /* its grow-only slab: x1 [np][3] */
  size_t cloud_bytes;
  int atm_cap;
  int atm_slices;               /* distinct time stamps in the atmosphere        */
  int atm_k_zero;               /* jur_atm_k_zero of the rows on the device (view.atm_k_zero: this, where the switch is on) */
  double atm_zmin, atm_zmax;    /* altitude range of the atmosphere on the device */
  /* per-call workspace */
  int chunk_rays;               /* R                                             */
  int nfield;
  double *d_los;
  double *d_eps;                /* segment transmittances per (channel, gas)     */
  long ws_budget;               /* bytes of workspace the model may hold         */
  long ws_rays;                 /* R: rays per ega/combine launch the workspace is laid out for */
  long ws_trace_rays;           /* Rt >= R: rays per trace launch (LOS workspace stride)        */
  int trace_mult;               /* wanted Rt / R                                                */
  long use_rays, use_trace_rays;/* R, Rt of the current call (<= the allocated capacities)     */
  int *d_np;
  double *d_tsurf;
  int compact_ws;               /* 1 (default): calls that need several integration launches lay the transmittance tiles
                                   out by the path lengths that occur instead of JUR_NLOS points per ray           */
  int use_compact;              /* ... and the current call does                                                 */
  int *d_tile_np, *d_eps_off;   /* [ws_trace_rays / 64] longest path per tile; first point slot of the tile in d_eps */
  int *h_tile;                  /* pinned: [2][ws_trace_rays / 64] host images of the two                        */
  long n_launch_ega;            /* integration launches of the last batched call (reporting)                     */
  int *d_status;
  long los_bytes;
  /* ray ordering */
  int sort_rays;                /* 1: process rays in order of tangent altitude  */
  int *d_order;
  void *d_sort_tmp;
  long order_cap, sort_tmp_bytes;
  int *d_blk_order;             /* [(order_cap + 255) / 256] blocks of 256 sorted slots, longest paths first (see
                                   formod_device_body)                                                       */
  long n_blk_order;             /* blocks of the last batched call's order, 0: it built none                  */
  /* staging for the host entry */
  double *d_io;                 /* geom[7][cap] tp[3][cap] rad/tau[cap][nd]      */
  int *d_io_np;
  long io_cap;
  int *h_status;                /* pinned: the device status word comes back here (a pageable target would make the
                                   copy a blocking one inside the runtime and serialise concurrent callers)      */
  double *h_io;                 /* pinned host image of d_io (+ np behind it) for callers with pageable arrays */
  long h_io_cap;
  double *h_pkg;                /* pinned scratch of the drop-in entry: rad/tau of one package, [2][NR][nd] */
  double *h_atm;                /* host image of the atmosphere rows last uploaded (after the hydrostatic step) */
  long h_atm_n, h_atm_cap;
  double h_atm_hydz;
  hipStream_t stream;
  hipStream_t stream2;          /* copies that run beside the kernels of `stream` */
  hipEvent_t ev_mask, ev_trace;
  int host_call;                /* 1 while jur_formod_host drives jur_formod_device: record / wait for the events above */
  hipEvent_t ev_done;           /* recorded on the caller's stream at the end of every jur_formod_device call: what a
                                   later upload of the atmosphere waits for (no handle of the caller's is kept) */
  int have_done;
  /* field-of-view convolution of device arrays: grow-only scratch and its own status word */
  double *d_fov;
  long fov_cap;
  /* field of view of the scene entries (jur_model_set_fov): the shape on the host and dz | w on the device */
  int fov_n;
  double *fov_shape;            /* dz[JUR_NSHAPE] | w[JUR_NSHAPE], malloc'ed with the first shape */
  double *d_fov_shape;
  /* full a-priori precision of the slices (jur_model_set_prior_precision): the layout on the host, wptr | aptr and R on
   * the device; pp_nslice == 0: off */
  long pp_nslice;
  long *pp_wptr;                /* wptr[pp_nslice + 1] | aptr[pp_nslice + 1], malloc'ed */
  double *pp_R;                 /* host copy, what jur_model_prior_precision returns */
  void *d_pp;                   /* device: the same 2 (pp_nslice + 1) longs, then R */
  double scene_hydz;            /* hydrostatic balance of the scene entries per slice (jur_model_set_scene_hydz): the
                                   reference altitude [km], negative: off                                   */
  int kernel_recomp;            /* jur_retrieve_scene_host recomputes the Jacobian every n-th iteration (jur_model_set_kernel_recomp) */
  int scene_overflow;           /* JUR_OVERFLOW_*: what jur_trial_scene_host and jur_retrieve_scene_host make of an untraceable ray */
  long ov_cells, ov_failed;     /* ... and what the last of their calls counted (jur_model_last_scene_overflow) */
  int sb_nq;                    /* the box on the state (jur_model_set_state_bounds): 2 + ng + nw quantities, 0: off */
  double sb_lo[2 + JUR_NG + JUR_NW], sb_hi[2 + JUR_NG + JUR_NW];
  double *d_kq, *h_kq;          /* jur_kernel: perturbation steps and dense difference quotients (device, pinned host) */
  long kq_cap;
  /* small calls: the fused kernel (jur_pencil_kernel) instead of sort + three batched kernels */
  long pencil_rays;             /* calls of up to this many rays take it (0: never)             */
  int pencil_rb;                /* rays per workgroup (0: chosen from the call size)            */
  /* timing */
  int timing;
  hipEvent_t *evpool;           /* 2 events per timed launch                     */
  unsigned char *evkind;        /* 0 trace, 1 ega, 2 combine, 3 fused (pencil), 4 contributions, 5 scene Jacobian, 6 the chains of C per pass */
  int ntimed;
  double pencil_ms;
  long pencil_launches;
  double contrib_ms;            /* jur_contrib_kernel's share (kind 4), collected with the others */
  long contrib_launches;
  double *d_ctb;                /* jur_formod_contrib_host: grow-only device scratch rad_c | tau_c */
  long ctb_cap;
  void *d_scene;                /* jur_kernel_scene_host: grow-only device slab (base rows, descriptors, per-ray arrays, blocks of a pass) */
  size_t scene_bytes;
  void *d_side;                 /* jur_param_scene_host: grow-only device buffer beside the slab, for what outlives the body's
                                   calls (gain, effective weights, C, the parameter covariances, sigma_param, the layout) */
  size_t side_bytes;
  double scene_ms;              /* its kernels' share (kinds 5 and 6), collected with the others */
  long scene_launches;
  double cross_ms;              /* ... of which jur_scene_cross_pass_kernel's (kind 6) */
  long cross_launches;
};

#define JUR_MAX_TIMED 4096

static int pencil_rays_per_group(jur_model_t const *m, long nr);

static int find_emitter(ctl_t const *ctl, char const *name) {
  for (int ig = 0; ig < ctl->ng; ig++)
    if (0 == strcasecmp(ctl->emitter[ig], name)) return ig;
  return -1;
}

static int upload(void **dst, void const *src, size_t bytes) {
  if (bytes == 0) bytes = 8;
  HIPCHK(hipMalloc(dst, bytes));
  if (src) HIPCHK(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
  return JUR_OK;
}

static int check_ctl(ctl_t const *ctl) {
  if (ctl->ng < 0 || ctl->ng > JUR_NG) { jur_set_error("ctl->ng=%d outside 0..%d", ctl->ng, JUR_NG); return JUR_EINVAL; }
  if (ctl->nd < 1 || ctl->nd > JUR_ND) { jur_set_error("ctl->nd=%d outside 1..%d", ctl->nd, JUR_ND); return JUR_EINVAL; }
  if (ctl->nw < 0 || ctl->nw > JUR_NW) { jur_set_error("ctl->nw=%d outside 0..%d", ctl->nw, JUR_NW); return JUR_EINVAL; }
  if (ctl->ip != 1 && ctl->ip != 2 && ctl->ip != 3) { jur_set_error("Unknown interpolation method, check IP! (ctl->ip == %d; 1, 2 or 3)", ctl->ip); return JUR_EINVAL; }
  if (ctl->ip == 3 && !(ctl->cx > 0 && isfinite(ctl->cx) && ctl->cz > 0 && isfinite(ctl->cz))) {
    jur_set_error("IP 3 (point cloud) needs finite influence lengths CX > 0 and CZ > 0 [km]: ctl->cx = %g, ctl->cz = %g", ctl->cx, ctl->cz);
    return JUR_EINVAL;
  }
  for (int id = 0; id < ctl->nd; id++)
    if (ctl->window[id] < 0 || ctl->window[id] >= (ctl->nw > 0 ? ctl->nw : 1)) { jur_set_error("ctl->window[%d] out of range", id); return JUR_EINVAL; }
  return JUR_OK;
}

static int create_streams(jur_model_t *m) {
  if (hipHostMalloc((void **)&m->h_status, 64, hipHostMallocDefault) != hipSuccess ||
      hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&m->stream2, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&m->ev_mask, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&m->ev_trace, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&m->ev_done, hipEventDisableTiming) != hipSuccess) {
    jur_set_error("cannot create the model's streams and events");
    return JUR_EHIP;
  }
  return JUR_OK;
}

int jur_model_create(jur_model_t **out, ctl_t const *ctl, jur_tables_t const *tb, int device) {
  *out = NULL;
  int rc = check_ctl(ctl);
  if (rc) return rc;
  if (!tb || tb->ng < ctl->ng || tb->nd < ctl->nd) { jur_set_error("tables do not cover ctl (ng, nd)"); return JUR_EINVAL; }
  for (int id = 0; id < ctl->nd; id++)
    if (!tb->have_sr[id]) { jur_set_error("no filter function / source table for channel %d", id); return JUR_EINVAL; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { jur_set_error("no HIP device available"); return JUR_ENODEV; }
  if (device < 0 || device >= ndev) { jur_set_error("device %d not in 0..%d", device, ndev - 1); return JUR_ENODEV; }
  HIPCHK(hipSetDevice(device));

  jur_model_t *m = (jur_model_t *)calloc(1, sizeof *m);
  if (!m) return JUR_ENOMEM;
  m->device = device;
  m->scene_hydz = -1;
  m->kernel_recomp = 1;
  m->ctl = (ctl_t *)malloc(sizeof(ctl_t));
  if (!m->ctl) { free(m); return JUR_ENOMEM; }
  memcpy(m->ctl, ctl, sizeof(ctl_t));
  m->track.ip = ctl->ip;
  m->cloud.cx = ctl->cx; m->cloud.cz = ctl->cz;
  jur_view_t *v = &m->view;
  v->ng = ctl->ng; v->nd = ctl->nd; v->nw = ctl->nw > 0 ? ctl->nw : 1;
  v->refrac = ctl->refrac; v->write_bbt = ctl->write_bbt;
  v->rayds = ctl->rayds; v->raydz = ctl->raydz;
  /* continuum switches, CPUdrivers.c:126-134 */
  v->ig_co2 = -999; v->ig_h2o = -999;
  if (ctl->ctm_h2o) v->ig_h2o = find_emitter(ctl, "H2O");
  if (ctl->ctm_co2) v->ig_co2 = find_emitter(ctl, "CO2");
  v->fourbit = ((1 == ctl->ctm_co2) && (v->ig_co2 >= 0)) * 8 + ((1 == ctl->ctm_h2o) && (v->ig_h2o >= 0)) * 4
             + (1 == ctl->ctm_n2) * 2 + (1 == ctl->ctm_o2) * 1;

  jur_chan_t *chan = (jur_chan_t *)calloc(ctl->nd, sizeof(jur_chan_t));
  if (!chan) { jur_model_destroy(m); return JUR_ENOMEM; }
  for (int id = 0; id < ctl->nd; id++)
    if ((rc = jur_chan_setup(&chan[id], ctl->nu[id], ctl->window[id]))) { free(chan); jur_model_destroy(m); return rc; }
  rc = upload(&m->d_chan, chan, sizeof(jur_chan_t) * ctl->nd);
  free(chan);
  if (rc) { jur_model_destroy(m); return rc; }
  if ((rc = upload(&m->d_sr, tb->sr, sizeof(double) * JUR_TBLNS * ctl->nd))) { jur_model_destroy(m); return rc; }

  /* tables restricted to the (ng, nd) the control block uses */
  jur_tables_t sub = *tb;
  jur_pair_t *subpair = NULL;
  if (tb->nd != ctl->nd || tb->ng != ctl->ng) {
    subpair = (jur_pair_t *)calloc((size_t)ctl->ng * ctl->nd + 1, sizeof(jur_pair_t));
    if (!subpair) { jur_model_destroy(m); return JUR_ENOMEM; }
    for (int g = 0; g < ctl->ng; g++)
      for (int d = 0; d < ctl->nd; d++) subpair[(size_t)g * ctl->nd + d] = tb->pair[(size_t)g * tb->nd + d];
    sub.pair = subpair; sub.ng = ctl->ng; sub.nd = ctl->nd;
  }
  jur_flat_t fl;
  rc = jur_tables_flatten(&sub, &fl);
  free(subpair);
  if (rc) { jur_model_destroy(m); return rc; }
  long const npair = (long)ctl->ng * ctl->nd;
  rc = upload(&m->d_pair, fl.pair, sizeof(jur_int2) * (npair > 0 ? npair : 1));
  if (!rc) rc = upload(&m->d_pair_e0, fl.pair_e0, sizeof(long long) * (npair > 0 ? npair : 1));
  if (!rc) rc = upload(&m->d_lvl, fl.lvl, sizeof(jur_lvl_t) * (fl.nlevel + 2));
  if (!rc) rc = upload(&m->d_crv, fl.crv, sizeof(jur_crv_t) * (fl.ncurve + 2));
  if (!rc) rc = upload(&m->d_ue, fl.ue, sizeof(jur_ue_t) * (fl.nentry + 2));
  if (!rc && fl.strict) {       /* bracket records for the strict-table look-up: entries i, i+1 and both slopes in 32 bytes */
    rc = upload(&m->d_rec, NULL, sizeof(jur_rec_t) * (fl.nentry + 2));
    if (!rc && (jurk_fill_records((jur_ue_t const *)m->d_ue, (jur_rec_t *)m->d_rec, fl.nentry + 1, NULL) ||
                hipStreamSynchronize(NULL) != hipSuccess)) {
      jur_set_error("cannot form the bracket records of the tables");
      rc = JUR_EHIP;
    }
    v->rec = (jur_rec_t const *)m->d_rec;
  }
  v->sorted_tables = fl.sorted;
  v->strict_tables = fl.strict;
  v->max_pair_curves = fl.max_pair_curves;
  m->table_bytes = (long)((sizeof(jur_ue_t) + (m->d_rec ? sizeof(jur_rec_t) : 0)) * fl.nentry + 16 * fl.ncurve + 16 * fl.nlevel + 8 * npair);
  jur_flat_free(&fl);
  if (rc) { jur_model_destroy(m); return rc; }
  v->chan = (jur_chan_t const *)m->d_chan;
  v->sr = (double const *)m->d_sr;
  v->pair = (jur_int2 const *)m->d_pair;
  v->pair_e0 = (long long const *)m->d_pair_e0;
  v->lvl = (jur_lvl_t const *)m->d_lvl;
  v->crv = (jur_crv_t const *)m->d_crv;
  v->ue = (jur_ue_t const *)m->d_ue;
  if ((rc = jur_model_set_arithmetic(m, getenv("JUR_EGA_NO_RCP") ? JUR_ARITH_EXACT : JUR_ARITH_FAST))) { jur_model_destroy(m); return rc; }

  m->nfield = JUR_F_K + v->nw + v->ng;
  m->chunk_rays = 1 << 21;      /* upper bound; the workspace budget sets the real size (1.4 M rays for 96 KB per ray).
                                   Measured: 7.7 M rays/s at 1 M rays per launch vs 6.8 M at 131072 (tails, launch fill) */
  m->sort_rays = 1;
  m->ws_budget = 128L << 30;    /* of 288 GB HBM; C3 needs 96 KB per ray */
  m->compact_ws = getenv("JUR_NO_COMPACT_WS") ? 0 : 1;
  m->trace_mult = 1;
  m->pencil_rays = 10000;       /* measured crossover with the batched kernels (4 channels x 5 emitters) */
  m->pencil_rb = 0;
  if (getenv("JUR_PENCIL_RAYS")) m->pencil_rays = atol(getenv("JUR_PENCIL_RAYS"));
  if (getenv("JUR_PENCIL_RB")) m->pencil_rb = atoi(getenv("JUR_PENCIL_RB"));
  /* tuning overrides for experiments; the setters of the API do the same */
  if (getenv("JUR_CHUNK_RAYS") && atoi(getenv("JUR_CHUNK_RAYS")) >= 64) m->chunk_rays = (atoi(getenv("JUR_CHUNK_RAYS")) + 63) / 64 * 64;
  if (getenv("JUR_TRACE_MULT") && atoi(getenv("JUR_TRACE_MULT")) >= 1) m->trace_mult = atoi(getenv("JUR_TRACE_MULT"));
  if (getenv("JUR_WS_GIB") && atoi(getenv("JUR_WS_GIB")) >= 1) m->ws_budget = (long)atoi(getenv("JUR_WS_GIB")) << 30;
  if ((rc = create_streams(m))) { jur_model_destroy(m); return rc; }
  if ((rc = upload((void **)&m->d_status, NULL, sizeof(int)))) { jur_model_destroy(m); return rc; }
  if (hipMemset(m->d_status, 0, sizeof(int)) != hipSuccess) { jur_set_error("cannot clear the status word"); jur_model_destroy(m); return JUR_EHIP; }
  *out = m;
  return JUR_OK;
}

/* JUR_ARITH_FAST (default): on strictly increasing tables whose descriptors fit the LDS staging the look-up uses the
 * bracket records (both entries and both slopes of a bracket), reciprocal bracket widths and carries the path
 * transmittance as 1 - eps (~1e-13 from the reference's divisions); JUR_ARITH_EXACT: the reference's divisions operand
 * for operand (what every other table gets anyway).  Takes effect with the next call; calls in flight are the caller's
 * to wait for. */
int jur_model_set_arithmetic(jur_model_t *m, int mode) {
  if (mode != JUR_ARITH_FAST && mode != JUR_ARITH_EXACT) { jur_set_error("set_arithmetic: JUR_ARITH_FAST or JUR_ARITH_EXACT"); return JUR_EINVAL; }
  jur_view_t *v = &m->view;
  /* (the staging size of jurk_launch_ega: 24 B per level and curve of the largest pair, at most 48 KB) */
  int const lds_ok = v->max_pair_curves > 0 && 24L * JUR_TBLNP + 24L * v->max_pair_curves <= 48 * 1024;
  m->arith = mode;
  v->fast_arith = (mode == JUR_ARITH_FAST) && v->strict_tables && v->rec && lds_ok;
  return JUR_OK;
}
int jur_model_arithmetic(jur_model_t const *m) { return m->arith; }

int jur_model_create_from_files(jur_model_t **out, ctl_t const *ctl, int device) {
  *out = NULL;
  int rc = check_ctl(ctl);
  if (rc) return rc;
  /* READ_BINARY / WRITE_BINARY as upstream's init_tbl (jurassic.c:312-320, 669-671): != 0 try the
   * cache first, > 0 insist on it; write it after parsing the ASCII files when WRITE_BINARY != 0. */
  char cache[256];
  jur_tables_cache_filename(cache, sizeof cache, ctl);
  jur_tables_t *tb = NULL;
  if (ctl->read_binary) {
    rc = jur_tables_load(&tb, ctl, cache);
    if (rc == JUR_OK) printf("matching binary tables file found\n");
    else if (ctl->read_binary > 0) return rc;
  }
  if (!tb) {
    tb = jur_tables_new(ctl->ng, ctl->nd);
    if (!tb) return JUR_ENOMEM;
    rc = jur_tables_read_ascii(tb, ctl);
    if (rc >= 0) {
      int const found = rc;
      if (found < ctl->ng * ctl->nd) printf("Warning! %d files were not found!\n", ctl->ng * ctl->nd - found);
      rc = jur_tables_read_filters(tb, ctl);
    }
    if (rc == JUR_OK && ctl->write_binary && jur_tables_save(tb, ctl, cache) != JUR_OK)
      printf("Warning! could not write %s: %s\n", cache, jur_last_error());
  }
  if (rc == JUR_OK) rc = jur_model_create(out, ctl, tb, device);
  jur_tables_free(tb);
  return rc;
}

void jur_model_destroy(jur_model_t *m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  if (m->shared_tables) m->d_chan = m->d_sr = m->d_pair = m->d_pair_e0 = m->d_lvl = m->d_crv = m->d_ue = m->d_rec = NULL;
  void *ptrs[] = {m->d_chan, m->d_sr, m->d_pair, m->d_pair_e0, m->d_lvl, m->d_crv, m->d_ue, m->d_rec, m->d_atm, m->d_track, m->d_cloud, m->d_order, m->d_sort_tmp, m->d_blk_order,
                  m->d_los, m->d_eps, m->d_np, m->d_tsurf, m->d_status, m->d_io, m->d_io_np, m->d_fov, m->d_fov_shape, m->d_kq, m->d_ctb, m->d_scene, m->d_side, m->d_pp};
  for (size_t i = 0; i < sizeof ptrs / sizeof ptrs[0]; i++)
    if (ptrs[i]) (void)hipFree(ptrs[i]);
  if (m->h_io) (void)hipHostFree(m->h_io);
  if (m->h_pkg) (void)hipHostFree(m->h_pkg);
  if (m->h_kq) (void)hipHostFree(m->h_kq);
  if (m->h_status) (void)hipHostFree(m->h_status);
  free(m->h_atm);
  free(m->fov_shape);
  free(m->pp_wptr);
  free(m->pp_R);
  if (m->stream) (void)hipStreamDestroy(m->stream);
  if (m->stream2) (void)hipStreamDestroy(m->stream2);
  if (m->ev_mask) (void)hipEventDestroy(m->ev_mask);
  if (m->ev_trace) (void)hipEventDestroy(m->ev_trace);
  if (m->ev_done) (void)hipEventDestroy(m->ev_done);
  if (m->evpool) {
    for (int i = 0; i < 2 * JUR_MAX_TIMED; i++) (void)hipEventDestroy(m->evpool[i]);
    free(m->evpool);
    free(m->evkind);
  }
  free(m->ctl);
  free(m);
}

/* ---- hydrostatic adjustment on the host (jr_common.h:212-217, 713-761) ------ */
/* (the arithmetic is jur_hydrostatic_profile's, jur_scene.c: one text for formod()'s adjustment and the scene entries') */
static void hydrostatic(ctl_t const *ctl, int ig_h2o, int n, double const *z, double const *lat, double const *t,
                        double const *qh2o, double *p) {
  jur_hydrostatic_profile(ctl->hydz, n, z, lat, t, (ig_h2o >= 0) ? qh2o : NULL, p);
}

/* Host image of an atmosphere: rows time, z, lon, lat, p, T, q[ng], k[nw], each n long. */
static void pack_atm_rows(jur_model_t const *m, atm_t const *atm, double *h, size_t stride, size_t at) {
  int const n = atm->np, ng = m->view.ng, nw = m->view.nw;
  memcpy(h + 0 * stride + at, atm->time, sizeof(double) * n);
  memcpy(h + 1 * stride + at, atm->z, sizeof(double) * n);
  memcpy(h + 2 * stride + at, atm->lon, sizeof(double) * n);
  memcpy(h + 3 * stride + at, atm->lat, sizeof(double) * n);
  memcpy(h + 4 * stride + at, atm->p, sizeof(double) * n);
  memcpy(h + 5 * stride + at, atm->t, sizeof(double) * n);
  for (int g = 0; g < ng; g++) memcpy(h + (6 + (size_t)g) * stride + at, atm->q[g], sizeof(double) * n);
  for (int w = 0; w < nw; w++) memcpy(h + (6 + (size_t)ng + w) * stride + at, atm->k[w], sizeof(double) * n);
}

/* hydrostatic adjustment of one packed atmosphere of n points starting at `at` (CPUdrivers.c:98-103) */
static void hydrostatic_rows(jur_model_t const *m, double *h, size_t stride, size_t at, int n) {
  if (m->ctl->hydz < 0) return;
  int const ig = m->view.ig_h2o;
  hydrostatic(m->ctl, ig, n, h + 1 * stride + at, h + 3 * stride + at, h + 5 * stride + at,
              ig >= 0 ? h + (6 + (size_t)ig) * stride + at : NULL, h + 4 * stride + at);
}

/* Time stamps of an atmosphere of n points stacked behind others (kernel_ld, contrib_hydrostatic), shifted by `shift`.
 * Stacked, its end points are no longer the ends of the array, where locate_atm lets one point alone join the slice
 * next to it (jr_common.h:127-154): such a point takes that slice's time stamp, and the two points of a two-point
 * atmosphere (every ray's slice alone) one time stamp.  Then every slice of two or more points that a ray meets in
 * the atmosphere alone is a run of equal time stamps of the block (time stamps sorted; unsorted ones make locate_atm's
 * bisection depend on the array's length, and no stacking reproduces it).  In place is allowed. */
static void stack_times(double *dst, double const *src, int n, double shift) {
  double const first = (n >= 2 && src[0] != src[1]) ? src[1] : src[0];
  double const last = (n >= 3 && src[n - 1] != src[n - 2]) ? src[n - 2] : (n == 2 ? first : src[n - 1]);
  for (int i = 1; i < n - 1; i++) dst[i] = src[i] + shift;
  dst[0] = first + shift;
  dst[n - 1] = last + shift;
}

/* Time stamp of a ray of a stacked block: the stacked time stamp (block_time, from stack_times) of the first point of
 * the slice the ray has in the atmosphere alone (time, n points), so that it finds the same points there -- also where
 * its own time stamp matches no profile but locate_atm still hands it two points or more.  A ray whose slice alone is
 * one point (not entered) gets `above`, a time stamp above all, and with it the last point alone. */
static double stacked_ray_time(double const *time, int n, double t, double const *block_time, double above) {
  long first;
  return jur_atm_slice(time, n, t, &first) >= 2 ? block_time[first] : above;
}

/* what the kernels want to know about the n points with time stamps `time` and altitudes `z` */
static void derive_atm_facts(jur_model_t *m, double const *time, double const *z, long n) {
  jur_view_t *v = &m->view;
  m->atm_slices = 1;
  m->atm_zmin = m->atm_zmax = z[0];
  for (long i = 1; i < n; i++) { if (z[i] < m->atm_zmin) m->atm_zmin = z[i]; if (z[i] > m->atm_zmax) m->atm_zmax = z[i]; }
  v->atm_sorted = 1;
  v->atm_maxslice = 1;
  for (long i = 1; i < n; i++) {
    if (time[i] != time[i - 1]) m->atm_slices++;
    if (time[i] < time[i - 1]) v->atm_sorted = 0;
  }
  /* The slices are those locate_atm hands the rays whose time stamps match a profile -- not always the runs of equal
   * time stamps: one point alone at either end of the atmosphere joins the slice next to it (jr_common.h:127-154).
   * Ray time stamps that match no profile get one point, or the last two, which never needs a sorted axis. */
  for (long a = 0; a < n;) {
    long lo, b = a + 1;
    while (b < n && time[b] == time[a]) b++;
    int const len = jur_atm_slice(time, n, time[a], &lo);
    if (len > v->atm_maxslice) v->atm_maxslice = len;
    for (long i = lo + 2; i < lo + len; i++)            /* z strictly monotone inside the slice */
      if ((z[i] > z[i - 1]) != (z[lo + 1] > z[lo]) || z[i] == z[i - 1]) v->atm_sorted = 0;
    if (len >= 2 && z[lo + 1] == z[lo]) v->atm_sorted = 0;
    a = b;
  }
}

/* May the kernels leave the extinction out (jur_view_t::atm_k_zero)?  Only for rows the host holds as the caller set
 * them (origin JUR_ATM_CALLER), on a sorted atmosphere, with every one of the `count` extinction values +0.0 bit for
 * bit: -0.0, a denormal or a NaN clears it.  The rows of a perturbed stack (kernel(), the hydrostatic contribution
 * variants) and rows a kernel writes on the device never qualify, whatever they hold.  The sorted atmosphere is what
 * makes the tracer's interpolation of two zeros a +0.0 (see trace_ray): its brackets have a finite width that is not 0. */
int jur_atm_k_zero(double const *k, long count, int atm_sorted, int origin) {
  if (origin != JUR_ATM_CALLER || !atm_sorted || count < 0 || (count > 0 && !k)) return 0;
  for (long i = 0; i < count; i++) {
    unsigned long long bits;
    memcpy(&bits, &k[i], sizeof bits);
    if (bits) return 0;
  }
  return 1;
}

static int g_k_elision = -1;           /* 1: on, 0: off, -1: nothing set -- JUR_K_ELISION (A/B switch, read once) */
static int g_k_elision_env = -1;
void jur_tune_k_elision(int mode) { g_k_elision = mode < 0 ? -1 : (mode != 0); }
static int k_elision_on(void) {
  if (g_k_elision_env < 0) g_k_elision_env = getenv("JUR_K_ELISION") ? atoi(getenv("JUR_K_ELISION")) != 0 : 1;
  return g_k_elision >= 0 ? g_k_elision : g_k_elision_env;
}
/* what the kernels of the next launches see: before every launch that traces, so that a call's tracer and the readers
 * of its LOS rows agree even where the switch has been turned between two calls */
static void view_set_k_zero(jur_model_t *m) { m->view.atm_k_zero = m->atm_k_zero && k_elision_on(); }
int jur_model_k_zero(jur_model_t *m) { if (!m || m->view.atm_np < 2) return 0; view_set_k_zero(m); return m->view.atm_k_zero; }

/* Profile table of the packed rows under ip == 2 (jur_track_rows: the rule in jurassic_hip.h), rebuilt with every
 * atmosphere; its size changes from call to call, so the slab only grows.  Nobody reads the old table any more: the
 * caller has waited for the model's last call. */
static int upload_track(jur_model_t *m, double const *h, long n) {
  jur_track_t *t = &m->track;
  t->nprof = 0;
  size_t const cap = (size_t)n / 2 + 1;
  size_t const nd = 4 * cap, ni = 3 * cap + (size_t)n;
  char *buf = (char *)malloc(sizeof(double) * nd + sizeof(int) * ni);
  if (!buf) return JUR_ENOMEM;
  double *hx1 = (double *)buf, *hlat = hx1 + 3 * cap;
  int *hfirst = (int *)(buf + sizeof(double) * nd), *hlen = hfirst + cap, *hdir = hlen + cap, *hprof = hdir + cap;
  long const nx = jur_track_rows(n, h, h + (size_t)n, h + 2 * (size_t)n, h + 3 * (size_t)n, hfirst, hlen, (double (*)[3])hx1, NULL, hdir, hprof);
  if (nx < 0) { free(buf); return (int)nx; }
  for (long ix = 0; ix < nx; ix++) hlat[ix] = h[3 * (size_t)n + hfirst[ix]];
  size_t const bytes = sizeof(double) * nd + sizeof(int) * ni;
  if (bytes > m->track_bytes) {
    if (m->d_track) (void)hipFree(m->d_track);
    m->d_track = NULL;
    m->track_bytes = 0;
    if (hipMalloc(&m->d_track, bytes) != hipSuccess) { free(buf); jur_set_error("cannot allocate the profile table of the track"); return JUR_EHIP; }
    m->track_bytes = bytes;
  }
  hipError_t e = hipMemcpyAsync(m->d_track, buf, bytes, hipMemcpyHostToDevice, m->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
  free(buf);
  if (e != hipSuccess) { jur_set_error("cannot upload the profile table of the track: %s", hipGetErrorString(e)); return JUR_EHIP; }
  double const *dd = (double const *)m->d_track;
  int const *di = (int const *)((char const *)m->d_track + sizeof(double) * nd);
  t->x1 = dd; t->lat = dd + 3 * cap;
  t->first = di; t->len = di + cap; t->dir = di + 2 * cap; t->prof_of = di + 3 * cap;
  t->nprof = (int)nx;
  return JUR_OK;
}

/* Positions of the packed rows' points under ip == 3 (jur_cloud_rows: rule 3 in jurassic_hip.h), rebuilt with every
 * atmosphere; the slab only grows.  Nobody reads the old table any more: the caller has waited for the model's last call. */
static int upload_cloud(jur_model_t *m, double const *h, long n) {
  jur_cloud_t *t = &m->cloud;
  t->np = 0;
  size_t const bytes = sizeof(double) * 3 * (size_t)n;
  double *buf = (double *)malloc(bytes);
  if (!buf) return JUR_ENOMEM;
  long const nx = jur_cloud_rows(n, h + 2 * (size_t)n, h + 3 * (size_t)n, (double (*)[3])buf);
  if (nx < 0) { free(buf); return (int)nx; }
  if (bytes > m->cloud_bytes) {
    if (m->d_cloud) (void)hipFree(m->d_cloud);
    m->d_cloud = NULL;
    m->cloud_bytes = 0;
    if (hipMalloc(&m->d_cloud, bytes) != hipSuccess) { free(buf); jur_set_error("cannot allocate the position table of the cloud"); return JUR_EHIP; }
    m->cloud_bytes = bytes;
  }
  hipError_t e = hipMemcpyAsync(m->d_cloud, buf, bytes, hipMemcpyHostToDevice, m->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
  free(buf);
  if (e != hipSuccess) { jur_set_error("cannot upload the position table of the cloud: %s", hipGetErrorString(e)); return JUR_EHIP; }
  t->x1 = (double const *)m->d_cloud;
  t->cx = m->ctl->cx; t->cz = m->ctl->cz;
  t->np = (int)nx;
  return JUR_OK;
}

/* upload packed rows [6+ng+nw][n] and derive what the kernels want to know about them; origin: JUR_ATM_* */
static int upload_atm_rows(jur_model_t *m, double const *h, long n, int origin) {
  HIPCHK(hipSetDevice(m->device));
  jur_view_t *v = &m->view;
  int const ng = v->ng, nw = v->nw;
  size_t const nrow = 6 + (size_t)ng + nw;
  v->atm_np = 0;                /* until the rows are up: a failure below leaves the model without atmosphere */
  m->atm_k_zero = 0; v->atm_k_zero = 0;
  if (n > m->atm_cap) {
    if (m->d_atm) (void)hipFree(m->d_atm);
    m->d_atm = NULL;
    m->atm_cap = 0;
    HIPCHK(hipMalloc(&m->d_atm, sizeof(double) * (nrow + 1) * (size_t)n));   /* + one row for atm_pslope */
    m->atm_cap = n;
  }
  /* Kernels of an earlier jur_formod_device call may still be reading the atmosphere on the CALLER's stream: wait
   * for the event that call left behind on it.  The event is the model's own; the caller's stream may have been
   * destroyed since (destruction completes its work, and the event with it). */
  if (m->have_done) {
    HIPCHK(hipEventSynchronize(m->ev_done));
    m->have_done = 0;
  }
  if (m->track.ip == 2) {       /* before the rows go up: a refused track leaves the model without atmosphere */
    int const rt = upload_track(m, h, n);
    if (rt) return rt;
  }
  if (m->track.ip == 3) {
    int const rt = upload_cloud(m, h, n);
    if (rt) return rt;
  }
  HIPCHK(hipMemcpyAsync(m->d_atm, h, sizeof(double) * nrow * (size_t)n, hipMemcpyHostToDevice, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
  derive_atm_facts(m, h, h + (size_t)n, n);
  m->atm_k_zero = jur_atm_k_zero(h + (6 + (size_t)ng) * (size_t)n, (long)nw * n, v->atm_sorted, origin);
  if (m->track.ip == 3) m->atm_k_zero = 0;   /* a mean over no parcel is NaN, in the extinction as well: never elided */
  view_set_k_zero(m);
  double const *d = (double const *)m->d_atm;
  v->atm_np = (int)n;           /* (jurk_prepare_atm reads it) */
  v->atm_time = d; v->atm_z = d + (size_t)n; v->atm_lon = d + 2 * (size_t)n; v->atm_lat = d + 3 * (size_t)n;
  v->atm_p = d + 4 * (size_t)n; v->atm_t = d + 5 * (size_t)n;
  v->atm_q = d + 6 * (size_t)n; v->atm_k = d + (6 + (size_t)ng) * n;
  v->atm_pslope = d + nrow * (size_t)n;
  int const ek = jurk_prepare_atm(v, (double *)m->d_atm + nrow * (size_t)n, m->stream);
  if (ek || hipStreamSynchronize(m->stream) != hipSuccess) { v->atm_np = 0; jur_set_error("atm preparation kernel failed"); return JUR_EHIP; }
  return JUR_OK;
}

int jur_model_set_atm(jur_model_t *m, atm_t const *atm) {
  if (!m || !atm || atm->np < 2 || atm->np > JUR_NP) { jur_set_error("set_atm: need 2..%d atmospheric points", JUR_NP); return JUR_EINVAL; }
  int const n = atm->np;
  size_t const nrow = 6 + (size_t)m->view.ng + m->view.nw;
  double *h = (double *)malloc(sizeof(double) * nrow * n);
  if (!h) return JUR_ENOMEM;
  pack_atm_rows(m, atm, h, (size_t)n, 0);
  /* The same atmosphere again (a caller looping over observation packages, formod.c:100, or the lanes of the
   * drop-in entry): what is on the device already is what this upload would put there.  Compared before the
   * hydrostatic step, which is a function of these rows and ctl->hydz. */
  if (m->h_atm && m->h_atm_n == n && m->h_atm_hydz == m->ctl->hydz && m->view.atm_np == n &&
      0 == memcmp(m->h_atm, h, sizeof(double) * nrow * n)) {
    free(h);
    return JUR_OK;
  }
  if ((long)(nrow * n) > m->h_atm_cap) {
    free(m->h_atm);
    m->h_atm = (double *)malloc(sizeof(double) * nrow * n);
    m->h_atm_cap = m->h_atm ? (long)(nrow * n) : 0;
  }
  m->h_atm_n = 0;
  if (m->h_atm) { memcpy(m->h_atm, h, sizeof(double) * nrow * n); m->h_atm_n = n; m->h_atm_hydz = m->ctl->hydz; }
  hydrostatic_rows(m, h, (size_t)n, 0, n);   /* on the private copy; the caller's atm is not modified */
  int const rc = upload_atm_rows(m, h, n, JUR_ATM_CALLER);
  if (rc) m->h_atm_n = 0;
  free(h);
  return rc;
}

/* ---- workspace --------------------------------------------------------------- */
static void free_workspace(jur_model_t *m) {
  if (m->d_los) (void)hipFree(m->d_los);
  if (m->d_eps) (void)hipFree(m->d_eps);
  if (m->d_np) (void)hipFree(m->d_np);
  if (m->d_tsurf) (void)hipFree(m->d_tsurf);
  if (m->d_tile_np) (void)hipFree(m->d_tile_np);
  if (m->d_eps_off) (void)hipFree(m->d_eps_off);
  if (m->h_tile) (void)hipHostFree(m->h_tile);
  m->d_los = NULL; m->d_eps = NULL; m->d_np = NULL; m->d_tsurf = NULL; m->d_tile_np = NULL; m->d_eps_off = NULL; m->h_tile = NULL;
  m->los_bytes = 0; m->ws_rays = 0; m->ws_trace_rays = 0;
}

static int ensure_workspace(jur_model_t *m, long nr) {
  /* bytes per ray: LOS fields (per traced ray), one double per (channel, gas, point) (per integrated ray).
   * Tracing is latency-bound and wants many rays per launch, so its launches cover Rt = trace_mult * R rays
   * while the ega/combine launches cover R. */
  long const per_ray_los = (long)sizeof(double) * m->nfield * JUR_NLOS;
  long const per_ray_eps = (long)sizeof(double) * m->view.nd * (m->view.ng > 0 ? m->view.ng : 1) * JUR_NLOS;
  long budget = m->ws_budget;
  int asked = 0;
  for (int attempt = 0;; attempt++) {
    long R = m->chunk_rays;
    long const fit = budget / (per_ray_los + per_ray_eps);
    if (R > fit) R = fit / 64 * 64;
    if (R < 64) R = 64;
    if (nr <= R) R = (nr + 63) / 64 * 64;
    else {  /* several launches: equal shares instead of full chunks and a short tail */
      long const nchunk = (nr + R - 1) / R;
      R = ((nr + nchunk - 1) / nchunk + 63) / 64 * 64;
    }
    long mult = m->trace_mult > 0 ? m->trace_mult : 1;
    while (mult > 1 && (per_ray_los * mult + per_ray_eps) * R > budget) mult--;
    long Rt = R * mult;
    if (nr < Rt) Rt = (nr + R - 1) / R * R;
    int compact = 0;
    if (nr > R && m->compact_ws) {
      /* Several integration launches with JUR_NLOS points set aside per ray.  Rays rarely have that many (nadir
       * 181 .. 182, limb 122 .. 393 of 400: SURVEY.md section 6): trace as many rays as the budget allows first -- the
       * LOS rows are the small part -- and give the rest of it to the transmittances, whose tiles jur_formod_device
       * then lays out by the longest path of each tile.  R stays the capacity in rays of JUR_NLOS points. */
      long Rt_c = (nr + 63) / 64 * 64;
      if (per_ray_los * Rt_c > budget / 2) Rt_c = budget / 2 / per_ray_los / 64 * 64;
      long R_c = (budget - per_ray_los * Rt_c) / per_ray_eps / 64 * 64;
      if (R_c > m->chunk_rays) R_c = m->chunk_rays;            /* (the tuning knob: rays of JUR_NLOS points per launch) */
      if (R_c >= 64 && Rt_c >= R_c) { R = R_c; Rt = Rt_c; compact = 1; }
    }
    if (R <= m->ws_rays && Rt <= m->ws_trace_rays) {   /* the held workspace serves (smaller strides fit inside it) */
      m->use_rays = R;
      m->use_trace_rays = Rt;
      m->use_compact = compact;
      return JUR_OK;
    }
    if (!asked) {  /* about to allocate: never plan beyond what the device can give right now (another allocator
                      in the process may hold part of the HBM) */
      size_t free_b = 0, total_b = 0;
      asked = 1;
      if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        long const avail = (long)free_b + m->los_bytes - (2L << 30);
        if (avail > (64L << 20) && avail < budget) { budget = avail; continue; }
      } else (void)hipGetLastError();
    }
    free_workspace(m);
    hipError_t e = hipMalloc((void **)&m->d_los, (size_t)per_ray_los * Rt);
    if (e == hipSuccess) e = hipMalloc((void **)&m->d_eps, (size_t)per_ray_eps * R);
    if (e == hipSuccess) e = hipMalloc((void **)&m->d_np, sizeof(int) * Rt);
    if (e == hipSuccess) e = hipMalloc((void **)&m->d_tsurf, sizeof(double) * Rt);
    if (e == hipSuccess) e = hipMalloc((void **)&m->d_tile_np, sizeof(int) * (Rt / 64 + 1));
    if (e == hipSuccess) e = hipMalloc((void **)&m->d_eps_off, sizeof(int) * (Rt / 64 + 1));
    if (e == hipSuccess) e = hipHostMalloc((void **)&m->h_tile, sizeof(int) * 2 * (Rt / 64 + 1), hipHostMallocDefault);
    if (e == hipSuccess) {
      m->los_bytes = per_ray_los * Rt + per_ray_eps * R;
      m->ws_rays = R;
      m->ws_trace_rays = Rt;
      m->use_rays = R;
      m->use_trace_rays = Rt;
      m->use_compact = compact;
      return JUR_OK;
    }
    (void)hipGetLastError();
    free_workspace(m);
    if (R <= 64 || attempt >= 24) {
      jur_set_error("cannot allocate the workspace (%ld B per ray, even for %ld rays): %s", per_ray_los + per_ray_eps, R,
                    hipGetErrorString(e));
      return JUR_EHIP;
    }
    budget = (per_ray_los + per_ray_eps) * R / 2;   /* allocation refused: try again with half the rays per launch */
  }
}

long jur_model_workspace_bytes(jur_model_t const *m) { return m->los_bytes; }
long jur_model_scene_bytes(jur_model_t const *m) { return m ? (long)(m->scene_bytes + m->side_bytes) : 0; }
long jur_model_table_bytes(jur_model_t const *m) { return m->table_bytes; }

/* What a caller that plans its memory wants to know about a device before it allocates: PCI bus id (text), free and
 * total bytes right now. */
int jur_device_info(int device, char *pci_bus_id, int len, size_t *free_bytes, size_t *total_bytes) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { jur_set_error("device %d not available", device); return JUR_ENODEV; }
  HIPCHK(hipSetDevice(device));
  if (pci_bus_id && len > 0) HIPCHK(hipDeviceGetPCIBusId(pci_bus_id, len, device));
  size_t f = 0, t = 0;
  HIPCHK(hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = f;
  if (total_bytes) *total_bytes = t;
  return JUR_OK;
}
int jur_model_device(jur_model_t const *m) { return m->device; }
int jur_model_nd(jur_model_t const *m) { return m->view.nd; }
void *jur_model_stream(jur_model_t const *m) { return (void *)m->stream; }
int *jur_model_status_word(jur_model_t const *m) { return m->d_status; }
void jur_model_cost_params(jur_model_t const *m, double *rayds, double *raydz, double *zmin, double *zmax) {
  *rayds = m->view.rayds; *raydz = m->view.raydz; *zmin = m->atm_zmin; *zmax = m->atm_zmax;
}
int jur_model_chunk_rays(jur_model_t const *m) { return m->chunk_rays; }
long jur_model_last_launches(jur_model_t const *m) { return m->n_launch_ega; }
/* the block order of the last batched call (see formod_device_body), for tests and tools: waits for that call */
long jur_model_block_order(jur_model_t *m, int *out, long cap) {
  if (!m || m->n_blk_order <= 0) return 0;
  long const n = m->n_blk_order < cap ? m->n_blk_order : cap;
  if (hipSetDevice(m->device) != hipSuccess || (m->have_done && hipEventSynchronize(m->ev_done) != hipSuccess) ||
      (out && n > 0 && hipMemcpy(out, m->d_blk_order, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)) {
    (void)hipGetLastError();
    jur_set_error("block order: read-back failed");
    return JUR_EHIP;
  }
  return m->n_blk_order;
}
int jur_model_set_compact_workspace(jur_model_t *m, int on) { m->compact_ws = on ? 1 : 0; return JUR_OK; }

int jur_model_set_sort_rays(jur_model_t *m, int on) { m->sort_rays = on ? 1 : 0; return JUR_OK; }

int jur_model_set_workspace_budget(jur_model_t *m, long bytes) {
  if (bytes < (64L << 20)) { jur_set_error("workspace budget below 64 MiB"); return JUR_EINVAL; }
  m->ws_budget = bytes;
  return JUR_OK;
}

int jur_model_set_trace_multiple(jur_model_t *m, int mult) {
  if (mult < 1 || mult > 64) { jur_set_error("trace multiple must be in 1..64"); return JUR_EINVAL; }
  m->trace_mult = mult;
  return JUR_OK;
}

int jur_model_set_chunk_rays(jur_model_t *m, int rays) {
  if (rays < 64 || rays > (1 << 22)) { jur_set_error("chunk_rays must be in 64..4194304"); return JUR_EINVAL; }
  m->chunk_rays = (rays + 63) / 64 * 64;
  return JUR_OK;
}

int jur_model_set_pencil(jur_model_t *m, long max_rays, int rays_per_group) {
  if (max_rays < 0 || rays_per_group < 0 || rays_per_group > 64) { jur_set_error("set_pencil: max_rays >= 0, rays_per_group in 0..64"); return JUR_EINVAL; }
  m->pencil_rays = max_rays;
  m->pencil_rb = rays_per_group;
  return JUR_OK;
}

void jur_tune_trace(int lanes_per_ray) { jurk_tune_trace(lanes_per_ray); }
void jur_tune_trace_slice(int mode) { jurk_tune_trace_slice(mode); }
static int g_block_order = 0;          /* 0: by launch (see formod_device_body), 1: never, 2: whenever the rays were sorted */
void jur_tune_block_order(int mode) { g_block_order = (mode == 1 || mode == 2) ? mode : 0; }
/* ... or, where nothing has been set, JUR_BLOCK_ORDER (A/B switch, read once); JUR_BLOCK_ORDER_COMBINE=0 keeps the
 * radiance update in order (the ray tracer's share on its own) */
static int g_block_order_env = -1, g_block_order_combine = 1;
static int block_order_mode(void) {
  if (g_block_order_env < 0) {
    g_block_order_combine = getenv("JUR_BLOCK_ORDER_COMBINE") ? atoi(getenv("JUR_BLOCK_ORDER_COMBINE")) != 0 : 1;
    int const e = getenv("JUR_BLOCK_ORDER") ? atoi(getenv("JUR_BLOCK_ORDER")) : 0;
    g_block_order_env = (e == 1 || e == 2) ? e : 0;
  }
  return g_block_order ? g_block_order : g_block_order_env;
}

/* the look-up's share of the block order (it needs one built: jur_tune_block_order): 1 on, 0 the look-up in slot order,
 * < 0 back to JUR_BLOCK_ORDER_EGA (A/B switch, read once).  Off by default: measured, the look-up's event time does not
 * move with it (profiles/README.md, round 8) */
static int g_block_order_ega = -1, g_block_order_ega_env = -1;
void jur_tune_block_order_ega(int mode) { g_block_order_ega = mode < 0 ? -1 : (mode != 0); }
static int block_order_ega_on(void) {
  if (g_block_order_ega_env < 0) g_block_order_ega_env = getenv("JUR_BLOCK_ORDER_EGA") ? atoi(getenv("JUR_BLOCK_ORDER_EGA")) != 0 : 0;
  return g_block_order_ega >= 0 ? g_block_order_ega : g_block_order_ega_env;
}

void jur_tune_combine(int channels_per_group, int sync_segments, long min_lanes) {
  jurk_tune_combine(channels_per_group, sync_segments, min_lanes);
}

int jur_model_enable_timing(jur_model_t *m, int on) {
  HIPCHK(hipSetDevice(m->device));
  if (on && !m->evpool) {
    m->evpool = (hipEvent_t *)calloc(2 * JUR_MAX_TIMED, sizeof(hipEvent_t));
    m->evkind = (unsigned char *)calloc(JUR_MAX_TIMED, 1);
    if (!m->evpool || !m->evkind) return JUR_ENOMEM;
    for (int i = 0; i < 2 * JUR_MAX_TIMED; i++) HIPCHK(hipEventCreate(&m->evpool[i]));
  }
  m->timing = on;
  m->ntimed = 0;
  return JUR_OK;
}

/* Sums the event-bracketed durations of the launches recorded since the last
 * call (at most JUR_MAX_TIMED chunks), then starts over.
 * [0] trace, [1] ega, [2] combine. */
int jur_model_last_kernel_ms(jur_model_t *m, double out_ms[3], long out_launches[3]) {
  for (int k = 0; k < 3; k++) { out_ms[k] = 0; out_launches[k] = 0; }
  if (!m->evpool) return JUR_OK;
  HIPCHK(hipSetDevice(m->device));
  for (int i = 0; i < m->ntimed; i++) {
    float ms = 0;
    HIPCHK(hipEventSynchronize(m->evpool[2 * i + 1]));
    HIPCHK(hipEventElapsedTime(&ms, m->evpool[2 * i], m->evpool[2 * i + 1]));
    if (m->evkind[i] < 3) { out_ms[m->evkind[i]] += ms; out_launches[m->evkind[i]]++; }
    else if (m->evkind[i] == 3) { m->pencil_ms += ms; m->pencil_launches++; }
    else if (m->evkind[i] == 4) { m->contrib_ms += ms; m->contrib_launches++; }
    else {
      m->scene_ms += ms; m->scene_launches++;
      if (m->evkind[i] == 6) { m->cross_ms += ms; m->cross_launches++; }
    }
  }
  m->ntimed = 0;
  return JUR_OK;
}

/* the fused kernel's share of the launches timed since the last call of this function (call
 * jur_model_last_kernel_ms first: it collects the events) */
int jur_model_last_pencil_ms(jur_model_t *m, double *out_ms, long *out_launches) {
  *out_ms = m->pencil_ms;
  *out_launches = m->pencil_launches;
  m->pencil_ms = 0;
  m->pencil_launches = 0;
  return JUR_OK;
}

/* ... and of the contribution kernel (same protocol) */
int jur_model_last_contrib_ms(jur_model_t *m, double *out_ms, long *out_launches) {
  *out_ms = m->contrib_ms;
  *out_launches = m->contrib_launches;
  m->contrib_ms = 0;
  m->contrib_launches = 0;
  return JUR_OK;
}

/* ... and of the stacking, replication and quotient kernels of jur_kernel_scene_host (same protocol) */
int jur_model_last_scene_ms(jur_model_t *m, double *out_ms, long *out_launches) {
  *out_ms = m->scene_ms;
  *out_launches = m->scene_launches;
  m->scene_ms = 0;
  m->scene_launches = 0;
  return JUR_OK;
}

/* ... and, within that share, of jur_scene_cross_pass_kernel (jur_param_scene_host; same protocol) */
int jur_model_last_cross_ms(jur_model_t *m, double *out_ms, long *out_launches) {
  *out_ms = m->cross_ms;
  *out_launches = m->cross_launches;
  m->cross_ms = 0;
  m->cross_launches = 0;
  return JUR_OK;
}

static int ensure_sort_buffers(jur_model_t *m, long nr) {
  long const need = jurk_sort_tmp_bytes(nr);
  if (nr > m->order_cap || need > m->sort_tmp_bytes) {
    if (m->d_order) (void)hipFree(m->d_order);
    if (m->d_sort_tmp) (void)hipFree(m->d_sort_tmp);
    if (m->d_blk_order) (void)hipFree(m->d_blk_order);
    m->d_order = NULL; m->d_sort_tmp = NULL; m->d_blk_order = NULL; m->order_cap = 0; m->sort_tmp_bytes = 0;
    HIPCHK(hipMalloc((void **)&m->d_order, sizeof(int) * (size_t)nr));
    HIPCHK(hipMalloc((void **)&m->d_blk_order, sizeof(int) * (size_t)((nr + 255) / 256)));
    HIPCHK(hipMalloc(&m->d_sort_tmp, (size_t)need));
    m->order_cap = nr; m->sort_tmp_bytes = need;
  }
  return JUR_OK;
}

/* Allocate everything a later jur_formod_device(m, nr, ...) needs, so that the call itself only
 * enqueues kernels (it can then be captured into a HIP graph). */
int jur_model_reserve(jur_model_t *m, long nr) {
  if (!m || nr < 1 || nr > 0x7fffffffL) { jur_set_error("reserve: bad ray count"); return JUR_EINVAL; }
  HIPCHK(hipSetDevice(m->device));
  if (pencil_rays_per_group(m, nr) > 0) return JUR_OK;      /* the fused kernel keeps its state in LDS */
  int rc = ensure_workspace(m, nr);
  if (rc == JUR_OK && m->sort_rays && nr > 64) rc = ensure_sort_buffers(m, nr);
  return rc;
}

/* ---- forward model ------------------------------------------------------------ */
/* Rays per workgroup of the fused kernel for a call of nr rays, or 0 when the call goes to the batched kernels
 * (too many rays, or more (channel, gas) chains per ray than the LDS rings hold). */
static int pencil_rays_per_group(jur_model_t const *m, long nr) {
  if (m->ctl->formod == 1) return 0;                        /* the fused kernel is emissivity growth only */
  if (m->ctl->ip == 2 || m->ctl->ip == 3) return 0;         /* ... and traces one profile per ray */
  if (m->pencil_rays <= 0 || nr > m->pencil_rays) return 0;
  long const npair = (long)m->view.nd * (m->view.ng > 0 ? m->view.ng : 1);
  int rb = m->pencil_rb;
  if (rb <= 0) {
    /* Measured (tools/bench_small.py, profiles/r02_small_call_latency.json): with 10 chains per ray the fused kernel
     * beats the batched ones up to ~10 000 rays, with 20 up to ~4 500: the chains' look-ups (four lanes each) must
     * keep up with the tracer.  Rays per workgroup: about 136 workgroups per call and at most 8 rays for up to 12
     * chains per ray, 1 or 4 rays for up to 25, fewer beyond, so that a workgroup's chain lanes stay within its
     * eight look-up wavefronts. */
    if (nr * npair > 100000) return 0;
    if (npair <= 12) {
      rb = 1;
      while (rb < 8 && nr > 136L * rb) rb *= 2;
    } else if (npair <= 25) rb = (nr <= 600) ? 1 : 4;      /* (2 rays per workgroup measured slower than 1 and 4) */
    else rb = (npair <= 50 && nr > 600) ? 2 : 1;
  }
  if (rb > 64) rb = 64;
  while (rb > 1 && jurk_pencil_lds_bytes(&m->view, rb) <= 0) rb /= 2;
  return jurk_pencil_lds_bytes(&m->view, rb) > 0 ? rb : 0;
}

/* Leaves the model's event behind the work just enqueued on the caller's stream (see upload_atm_rows).  Not while
 * the stream is being captured into a graph: the graph's launches are the caller's to order against later uploads. */
static int record_done(jur_model_t *m, hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); st = hipStreamCaptureStatusNone; }
  if (st != hipStreamCaptureStatusNone) return JUR_OK;
  HIPCHK(hipEventRecord(m->ev_done, s));
  m->have_done = 1;
  return JUR_OK;
}

/* Every forward-model call of a model shares its workspace (LOS rows, transmittances, ray order, status word), and the
 * host entries, jur_kernel and jur_curtis_godson_host its I/O image too: before a call enqueues anything, its stream
 * waits for the event the last jur_formod_device call left behind, whichever stream that was on.  The event is then
 * recorded again behind this call, so the chain holds across any number of streams.  Not while the stream is being
 * captured: a graph cannot wait for work outside it; its launches are the caller's to order against other calls. */
static int wait_done(jur_model_t *m, hipStream_t s) {
  if (!m->have_done) return JUR_OK;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); st = hipStreamCaptureStatusNone; }
  if (st != hipStreamCaptureStatusNone) return JUR_OK;
  HIPCHK(hipStreamWaitEvent(s, m->ev_done, 0));
  return JUR_OK;
}

int jur_formod_device(jur_model_t *m, long nr, double const *d_geom, double *d_rad, double *d_tau, double *d_tp,
                      int *d_np, int *d_status, void *stream) {
  return jur_formod_device_ld(m, nr, d_geom, nr, d_rad, d_tau, d_tp, nr, d_np, d_status, stream);
}

/* where the contribution kernel writes (jur_formod_contrib_device): [ng + 1][nr][nd] each */
typedef struct { double *rad, *tau; } contrib_out_t;
static int formod_device_body(jur_model_t *m, long nr, double const *d_geom, long ldg, double *d_rad, double *d_tau, double *d_tp,
                              long ldtp, int *d_np, int *d_status, void *stream, contrib_out_t const *co);

int jur_formod_device_ld(jur_model_t *m, long nr, double const *d_geom, long ldg, double *d_rad, double *d_tau, double *d_tp,
                         long ldtp, int *d_np, int *d_status, void *stream) {
  return formod_device_body(m, nr, d_geom, ldg, d_rad, d_tau, d_tp, ldtp, d_np, d_status, stream, NULL);
}

/* The batched path; with `co` the contribution kernel runs after every look-up launch, on the plane it has just
 * written and before the radiance update overwrites the input radiances (the NaN mask).  Contributions never take the
 * fused kernel: it keeps no plane. */
static int formod_device_body(jur_model_t *m, long nr, double const *d_geom, long ldg, double *d_rad, double *d_tau, double *d_tp,
                              long ldtp, int *d_np, int *d_status, void *stream, contrib_out_t const *co) {
  if (!m || nr < 0) { jur_set_error("formod_device: bad arguments"); return JUR_EINVAL; }
  if (nr == 0) return JUR_OK;
  if (nr > 0x7fffffffL) { jur_set_error("formod_device: at most 2^31-1 rays per call"); return JUR_EINVAL; }
  if (m->view.atm_np < 2) { jur_set_error("formod_device: no atmosphere set"); return JUR_EINVAL; }
  view_set_k_zero(m);
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  int rc = wait_done(m, s);
  if (rc) return rc;
  int const rb = co ? 0 : pencil_rays_per_group(m, nr);
  if (rb > 0) {
    /* a package-sized call: the whole path in one launch, a workgroup per rb rays, LOS state in LDS */
    jur_chunk_t c;
    memset(&c, 0, sizeof c);
    c.n = (int)nr;
    for (int k = 0; k < 7; k++) c.geom[k] = d_geom + (size_t)k * ldg;
    for (int k = 0; k < 3; k++) c.tp[k] = d_tp + (size_t)k * ldtp;
    c.rad = d_rad;
    c.tau = d_tau;
    c.np_out = d_np;
    c.status = d_status ? d_status : m->d_status;
    if (m->host_call) HIPCHK(hipStreamWaitEvent(s, m->ev_mask, 0));
    int const ti = (m->timing && m->ntimed < JUR_MAX_TIMED) ? m->ntimed++ : -1;
    if (ti >= 0) { m->evkind[ti] = 3; HIPCHK(hipEventRecord(m->evpool[2 * ti], s)); }
    int const e = jurk_launch_pencil(&m->view, &c, rb, s);
    if (e) { jur_set_error("fused kernel launch failed: %s", hipGetErrorString((hipError_t)e)); return JUR_EHIP; }
    if (ti >= 0) HIPCHK(hipEventRecord(m->evpool[2 * ti + 1], s));
    if (m->host_call) HIPCHK(hipEventRecord(m->ev_trace, s));
    return record_done(m, s);
  }
  rc = ensure_workspace(m, nr);
  if (rc) return rc;
  long const R = m->use_rays;
  int const *order = NULL;
  int slice_sorted = m->atm_slices == 1;
  if (m->sort_rays && nr > 64) {
    /* similar rays side by side: equal trip counts inside a wavefront and neighbouring
     * table/profile addresses across its lanes */
    rc = ensure_sort_buffers(m, nr);
    if (rc) return rc;
    /* group by atmosphere slice when every slice is used by many rays */
    int const by_profile = m->atm_slices > 1 && nr >= 1024L * m->atm_slices;
    int const e = jurk_sort_rays(&m->view, by_profile, nr, d_geom, ldg, m->d_order, m->d_sort_tmp, m->sort_tmp_bytes, s);
    if (e) { jur_set_error("ray sort failed: %s", hipGetErrorString((hipError_t)e)); return JUR_EHIP; }
    order = m->d_order;
    slice_sorted |= by_profile;
  }
  long const Rt = m->use_trace_rays;
  /* Sorted slots ascend in tangent altitude within each profile, so a launch over them is a sawtooth of workgroup costs
   * (a limb ray at 3 km has four times the points of one at 68 km), handed out in blockIdx order: it ends with the long
   * workgroups of the last profiles on a mostly empty chip.  When the call is ONE trace launch, its blocks of 256 slots
   * are ordered by the tangent altitude of their lowest ray and the ray tracer, the look-up and the radiance update start them in
   * that order, longest first.  By default for launches the size of the slice tracer's (262 144 rays): below that the
   * chip is not filled several times over and the second sort is not paid for. */
  int const *blk_order = NULL;
  m->n_blk_order = 0;
  int const bo_mode = block_order_mode();
  if (order && nr <= Rt && bo_mode != 1 && (bo_mode == 2 || nr >= 4096L * 64)) {
    int const e = jurk_block_order(nr, m->d_blk_order, m->d_sort_tmp, m->sort_tmp_bytes, s);
    if (e) { jur_set_error("block order failed: %s", hipGetErrorString((hipError_t)e)); return JUR_EHIP; }
    blk_order = m->d_blk_order;
    m->n_blk_order = (nr + 255) / 256;
  }
  m->n_launch_ega = 0;
#define TIMED(kind, launch, what)                                                              \
  do {                                                                                         \
    int const ti_ = (m->timing && m->ntimed < JUR_MAX_TIMED) ? m->ntimed++ : -1;               \
    if (ti_ >= 0) { m->evkind[ti_] = (kind); HIPCHK(hipEventRecord(m->evpool[2 * ti_], s)); } \
    int const e_ = (launch);                                                                   \
    if (e_) { jur_set_error(what " kernel launch failed: %s", hipGetErrorString((hipError_t)e_)); return JUR_EHIP; } \
    if (ti_ >= 0) HIPCHK(hipEventRecord(m->evpool[2 * ti_ + 1], s));                          \
  } while (0)
  for (long t0 = 0; t0 < nr; t0 += Rt) {
    jur_chunk_t c;
    long const nt = (nr - t0 < Rt) ? nr - t0 : Rt;
    c.stride = (int)Rt;
    c.stride_eps = (int)R;
    for (int k = 0; k < 7; k++) c.geom[k] = d_geom + (size_t)k * ldg;
    for (int k = 0; k < 3; k++) c.tp[k] = d_tp + (size_t)k * ldtp;
    c.rad = d_rad;
    c.tau = d_tau;
    c.np_out = d_np;
    c.eps = m->d_eps;
    c.status = d_status ? d_status : m->d_status;
    c.slice_sorted = slice_sorted;
    /* trace the whole super-chunk */
    c.n = (int)nt;
    c.first = t0;
    c.order = order ? order + t0 : NULL;
    c.np = m->d_np;
    c.tsurf = m->d_tsurf;
    c.los = m->d_los;
    c.blk_order = blk_order;                          /* (set only where the call is this one launch) */
    TIMED(0, jurk_launch_trace(&m->view, &m->track, &m->cloud, &c, s), "trace");
    c.blk_order = NULL;
    if (m->host_call) {
      /* host entry: the input radiances, which only the epilogue reads (NaN mask), are uploaded beside the first
       * ray-tracing launch; tangent points and point counts are final after the last one and are copied out
       * beside the integration */
      if (t0 == 0) HIPCHK(hipStreamWaitEvent(s, m->ev_mask, 0));
      if (t0 + Rt >= nr) HIPCHK(hipEventRecord(m->ev_trace, s));
    }
    c.eps_off = NULL;
    int compact = m->use_compact && nt > R;
    if (compact) {   /* not while the stream is being captured: the layout needs the path lengths on the host */
      hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); st = hipStreamCaptureStatusNone; }
      if (st != hipStreamCaptureStatusNone) compact = 0;
    }
    if (compact) {
      /* Tiles laid out by the longest path of each (rays are sorted by tangent altitude: a tile's paths are nearly
       * equal): the longest path per tile comes back to the host -- the one wait of such a call --, consecutive tiles are
       * packed into launches of about equal size that fit the transmittance workspace, and every tile's first point
       * slot goes back up. */
      long const ntile = (nt + 63) / 64, cap = R / 64 * JUR_NLOS;      /* tile-points the workspace holds */
      int *const h_np = m->h_tile, *const h_off = m->h_tile + (m->ws_trace_rays / 64 + 1);
      int const ek = jurk_tile_max((int)nt, m->d_np, m->d_tile_np, s);
      if (ek) { jur_set_error("tile kernel launch failed: %s", hipGetErrorString((hipError_t)ek)); return JUR_EHIP; }
      HIPCHK(hipMemcpyAsync(h_np, m->d_tile_np, sizeof(int) * ntile, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      long total = 0;
      for (long t = 0; t < ntile; t++) total += h_np[t];
      long const nchunk = (total + cap - 1) / cap > 0 ? (total + cap - 1) / cap : 1;
      long const target = (total + nchunk - 1) / nchunk;               /* equal shares instead of full launches and a tail */
      /* first point slot of every tile, restarting per launch; a launch of many tiles ends on a multiple of 32 tiles
       * (8 ray blocks of 256 rays: one per XCD, see xcd_block_item in jur_kernels.hip) */
      for (long t = 0; t < ntile;) {
        long acc = 0, e = t;
        while (e < ntile && (e == t || (acc + h_np[e] <= cap && acc < target))) acc += h_np[e++];
        if (e < ntile && e - t >= 64) e = t + (e - t) / 32 * 32;
        acc = 0;
        for (long q = t; q < e; q++) { h_off[q] = (int)acc; acc += h_np[q]; h_np[q] = (q == t); }   /* (lengths not needed again: launch starts) */
        t = e;
      }
      HIPCHK(hipMemcpyAsync(m->d_eps_off, h_off, sizeof(int) * ntile, hipMemcpyHostToDevice, s));
      for (long t0c = 0; t0c < ntile;) {
        long t1c = t0c + 1;
        while (t1c < ntile && !h_np[t1c]) t1c++;
        long const s0 = t0c * 64, s1 = (t1c * 64 < nt) ? t1c * 64 : nt;
        c.n = (int)(s1 - s0);
        c.first = t0 + s0;
        c.order = order ? order + t0 + s0 : NULL;
        c.np = m->d_np + s0;
        c.tsurf = m->d_tsurf + s0;
        c.los = m->d_los + (size_t)s0 * JUR_NLOS * m->nfield;
        c.eps_off = m->d_eps_off + t0c;
        TIMED(1, jurk_launch_ega(&m->view, &c, m->ctl->formod == 1, s), "ega");
        if (co) TIMED(4, jurk_launch_contrib(&m->view, &c, nr, co->rad, co->tau, s), "contribution");
        TIMED(2, jurk_launch_combine(&m->view, &c, s), "combine");
        m->n_launch_ega++;
        t0c = t1c;
      }
      continue;
    }
    /* integrate it in chunks of R rays; slot s0 of the super-chunk is slot 0 of the chunk */
    for (long s0 = 0; s0 < nt; s0 += R) {
      c.n = (int)((nt - s0 < R) ? nt - s0 : R);
      c.first = t0 + s0;
      c.order = order ? order + t0 + s0 : NULL;
      c.np = m->d_np + s0;
      c.tsurf = m->d_tsurf + s0;
      c.los = m->d_los + (size_t)s0 * JUR_NLOS * m->nfield;   /* tiles of 64 slots, [tile][point][field][64]: s0 is a multiple of 64 */
      /* the look-up and the radiance update take the trace launch's block order where they cover the same slots */
      int const same_slots = blk_order && s0 == 0 && c.n == nt;
      if (same_slots && block_order_ega_on()) c.blk_order = blk_order;
      TIMED(1, jurk_launch_ega(&m->view, &c, m->ctl->formod == 1, s), "ega");
      c.blk_order = NULL;
      if (co) TIMED(4, jurk_launch_contrib(&m->view, &c, nr, co->rad, co->tau, s), "contribution");
      if (same_slots && g_block_order_combine) c.blk_order = blk_order;
      TIMED(2, jurk_launch_combine(&m->view, &c, s), "combine");
      c.blk_order = NULL;
      m->n_launch_ega++;
    }
  }
#undef TIMED
  return record_done(m, s);
}

/* ---- host entry ----------------------------------------------------------------- */
/* Pinned allocations for callers that want their arrays to travel at PCIe speed without staging. */
void *jur_host_alloc(size_t bytes) {
  void *p = NULL;
  if (hipHostMalloc(&p, bytes ? bytes : 8, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    jur_set_error("hipHostMalloc of %zu bytes failed", bytes);
    return NULL;
  }
  return p;
}
void jur_host_free(void *p) { if (p) (void)hipHostFree(p); }

static int is_pinned(void const *p) {
  hipPointerAttribute_t a;
  if (!p) return 0;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return a.type == hipMemoryTypeHost;
}

/* memcpy spread over a few host threads: a pageable array of a million rays moves at one core's ~10 GB/s otherwise */
typedef struct { char *dst; char const *src; size_t n; } cpjob_t;
static void *cp_worker(void *a) { cpjob_t const *j = (cpjob_t const *)a; memcpy(j->dst, j->src, j->n); return NULL; }
static void par_memcpy(void *dst, void const *src, size_t n) {
  enum { MAXT = 8 };
  int nt = 1;
  if (n >= ((size_t)4 << 20)) {
    long const ncpu = sysconf(_SC_NPROCESSORS_ONLN);
    nt = (int)(n >> 21);
    if (nt > MAXT) nt = MAXT;
    if (ncpu > 0 && nt > ncpu) nt = (int)ncpu;
  }
  if (nt <= 1) { memcpy(dst, src, n); return; }
  pthread_t th[MAXT];
  cpjob_t job[MAXT];
  size_t const per = ((n / nt) + 4095) & ~(size_t)4095;
  int started = 0;
  for (int i = 0; i < nt; i++) {
    size_t const o = per * i;
    if (o >= n) break;
    job[i].dst = (char *)dst + o; job[i].src = (char const *)src + o; job[i].n = (n - o < per) ? n - o : per;
    if (i == nt - 1 || o + per >= n || pthread_create(&th[started], NULL, cp_worker, &job[i]) != 0) {
      job[i].n = n - o;                          /* last share (or no thread to be had): the rest, here */
      memcpy(job[i].dst, job[i].src, job[i].n);
      break;
    }
    started++;
  }
  for (int i = 0; i < started; i++) pthread_join(th[i], NULL);
}

/* device / pinned-host images of one call's arrays:
 *   doubles: geom[7][nr] | rad[nr][nd] | tau[nr][nd] | tp[3][nr]   (inputs are a prefix, outputs a suffix)
 *   ints:    np[nr] */
static int ensure_io(jur_model_t *m, long nr, int want_host) {
  int const nd = m->view.nd;
  size_t const nval = (size_t)nr * (10 + 2 * (size_t)nd);
  if (nr > m->io_cap) {
    if (m->d_io) (void)hipFree(m->d_io);
    if (m->d_io_np) (void)hipFree(m->d_io_np);
    m->d_io = NULL; m->d_io_np = NULL; m->io_cap = 0;
    HIPCHK(hipMalloc((void **)&m->d_io, sizeof(double) * nval));
    HIPCHK(hipMalloc((void **)&m->d_io_np, sizeof(int) * (size_t)nr));
    m->io_cap = nr;
  }
  if (want_host && nr > m->h_io_cap) {
    if (m->h_io) (void)hipHostFree(m->h_io);
    m->h_io = NULL; m->h_io_cap = 0;
    HIPCHK(hipHostMalloc((void **)&m->h_io, sizeof(double) * nval + sizeof(int) * (size_t)nr, hipHostMallocDefault));
    m->h_io_cap = nr;
  }
  return JUR_OK;
}

int jur_model_io(jur_model_t *m, long nr, double **d_io, int **d_io_np) {
  HIPCHK(hipSetDevice(m->device));
  int const rc = ensure_io(m, nr, 0);
  if (rc) return rc;
  *d_io = m->d_io; *d_io_np = m->d_io_np;
  return JUR_OK;
}

#define JUR_SMALL_CALL 65536   /* rays: below this one staged transfer each way beats overlapping several */

int jur_formod_host(jur_model_t *m, long nr, double const *const geom[7], double *rad, double *tau, double *const tp[3],
                    int *np_out) {
  if (!m || nr < 0) { jur_set_error("formod_host: bad arguments"); return JUR_EINVAL; }
  if (nr == 0) return JUR_OK;
  HIPCHK(hipSetDevice(m->device));
  int const nd = m->view.nd;
  size_t const N = (size_t)nr, nrd = N * nd;
  hipStream_t const s = m->stream, s2 = m->stream2;
  int status = 0, rc;
  if ((rc = wait_done(m, s))) return rc;         /* a device-entry call on a stream of the caller's may still be running */

  if (nr <= JUR_SMALL_CALL) {
    /* a package: everything through the pinned image, one transfer in, one out */
    if ((rc = ensure_io(m, nr, 1))) return rc;
    double *const d_geom = m->d_io, *const d_rad = d_geom + 7 * N, *const d_tau = d_rad + nrd, *const d_tp = d_tau + nrd;
    double *const h_geom = m->h_io, *const h_rad = h_geom + 7 * N, *const h_tau = h_rad + nrd, *const h_tp = h_tau + nrd;
    int *const h_np = (int *)(h_tp + 3 * N);
    for (int k = 0; k < 7; k++) memcpy(h_geom + k * N, geom[k], sizeof(double) * N);
    memcpy(h_rad, rad, sizeof(double) * nrd);
    static int no_zero_copy = -1;                /* A/B switch, read once */
    if (no_zero_copy < 0) no_zero_copy = getenv("JUR_NO_ZERO_COPY") ? 1 : 0;
    if (pencil_rays_per_group(m, nr) > 0 && !no_zero_copy) {
      /* The fused kernel reads the geometry from the pinned image and writes its results there itself (a few
       * hundred KB over PCIe at the two ends of the kernel): ONE launch and one wait per call.  With copy
       * commands around the kernel, concurrent callers (the lanes of the drop-in entry) were serialised by the
       * runtime's copy path: 0.63 M rays/s with 16 threads against 1.9 M this way (tools/run_lanes_bench.sh). */
      *m->h_status = 0;
      if ((rc = jur_formod_device(m, nr, h_geom, h_rad, h_tau, h_tp, np_out ? h_np : NULL, m->h_status, s))) return rc;
    } else {
      HIPCHK(hipMemcpyAsync(d_geom, h_geom, sizeof(double) * (7 * N + nrd), hipMemcpyHostToDevice, s));
      HIPCHK(hipMemsetAsync(m->d_status, 0, sizeof(int), s));
      if ((rc = jur_formod_device(m, nr, d_geom, d_rad, d_tau, d_tp, m->d_io_np, m->d_status, s))) return rc;
      HIPCHK(hipMemcpyAsync(h_rad, d_rad, sizeof(double) * (2 * nrd + 3 * N), hipMemcpyDeviceToHost, s));
      if (np_out) HIPCHK(hipMemcpyAsync(h_np, m->d_io_np, sizeof(int) * N, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(m->h_status, m->d_status, sizeof(int), hipMemcpyDeviceToHost, s));
    }
    {  /* a package takes about a millisecond: poll instead of a wait that may sleep (in a process whose device is
        * set to blocking synchronisation -- PyTorch's default -- hipStreamSynchronize adds about 1 ms per call) */
      hipError_t q;
      int spins = 0;
      while ((q = hipStreamQuery(s)) == hipErrorNotReady)
        if (++spins > 2000) sched_yield();
      if (q != hipSuccess) { jur_set_error("HIP error %d (%s) while waiting for the package", (int)q, hipGetErrorString(q)); return JUR_EHIP; }
    }
    status = *m->h_status;
    memcpy(rad, h_rad, sizeof(double) * nrd);
    memcpy(tau, h_tau, sizeof(double) * nrd);
    for (int k = 0; k < 3; k++) memcpy(tp[k], h_tp + k * N, sizeof(double) * N);
    if (np_out) memcpy(np_out, h_np, sizeof(int) * N);
  } else {
    /* a batch: copies run beside the kernels on a second stream.  Arrays the caller keeps in pinned memory
     * (jur_host_alloc, hipHostMalloc, hipHostRegister) are transferred in place; pageable ones go through the
     * model's pinned image with a threaded memcpy.
     *   stream:  H2D geometry -> sort, trace | wait(mask) -> ega -> combine -> D2H rad, tau
     *   stream2: H2D input rad (NaN mask, read by the epilogue only) ........ wait(trace) -> D2H tp, np    */
    int pin_g[7], pin_tp[3], stage = 0;
    for (int k = 0; k < 7; k++) stage |= !(pin_g[k] = is_pinned(geom[k]));
    for (int k = 0; k < 3; k++) stage |= !(pin_tp[k] = is_pinned(tp[k]));
    int const pin_rad = is_pinned(rad), pin_tau = is_pinned(tau), pin_np = np_out ? is_pinned(np_out) : 1;
    stage |= !pin_rad | !pin_tau | !pin_np;
    if ((rc = ensure_io(m, nr, stage))) return rc;
    double *const d_geom = m->d_io, *const d_rad = d_geom + 7 * N, *const d_tau = d_rad + nrd, *const d_tp = d_tau + nrd;
    double *const h_geom = m->h_io, *const h_rad = h_geom ? h_geom + 7 * N : NULL, *const h_tau = h_geom ? h_rad + nrd : NULL,
           *const h_tp = h_geom ? h_tau + nrd : NULL;
    int *const h_np = h_geom ? (int *)(h_tp + 3 * N) : NULL;
    for (int k = 0; k < 7; k++) {
      double const *src = geom[k];
      if (!pin_g[k]) { par_memcpy(h_geom + k * N, geom[k], sizeof(double) * N); src = h_geom + k * N; }
      HIPCHK(hipMemcpyAsync(d_geom + k * N, src, sizeof(double) * N, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemsetAsync(m->d_status, 0, sizeof(int), s));
    {
      double const *src = rad;
      if (!pin_rad) { par_memcpy(h_rad, rad, sizeof(double) * nrd); src = h_rad; }
      HIPCHK(hipMemcpyAsync(d_rad, src, sizeof(double) * nrd, hipMemcpyHostToDevice, s2));
      HIPCHK(hipEventRecord(m->ev_mask, s2));
    }
    m->host_call = 1;
    rc = jur_formod_device(m, nr, d_geom, d_rad, d_tau, d_tp, m->d_io_np, m->d_status, s);
    m->host_call = 0;
    if (rc) { (void)hipStreamSynchronize(s2); return rc; }
    HIPCHK(hipStreamWaitEvent(s2, m->ev_trace, 0));
    for (int k = 0; k < 3; k++)
      HIPCHK(hipMemcpyAsync(pin_tp[k] ? tp[k] : h_tp + k * N, d_tp + k * N, sizeof(double) * N, hipMemcpyDeviceToHost, s2));
    if (np_out) HIPCHK(hipMemcpyAsync(pin_np ? np_out : h_np, m->d_io_np, sizeof(int) * N, hipMemcpyDeviceToHost, s2));
    HIPCHK(hipMemcpyAsync(pin_rad ? rad : h_rad, d_rad, sizeof(double) * nrd, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(pin_tau ? tau : h_tau, d_tau, sizeof(double) * nrd, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(m->h_status, m->d_status, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s2));             /* tangent points are here while the integration still runs */
    for (int k = 0; k < 3; k++)
      if (!pin_tp[k]) par_memcpy(tp[k], h_tp + k * N, sizeof(double) * N);
    if (np_out && !pin_np) par_memcpy(np_out, h_np, sizeof(int) * N);
    HIPCHK(hipStreamSynchronize(s));
    status = *m->h_status;
    if (!pin_rad) par_memcpy(rad, h_rad, sizeof(double) * nrd);
    if (!pin_tau) par_memcpy(tau, h_tau, sizeof(double) * nrd);
  }
  if (status & 1) { jur_set_error("Too many LOS points! (a ray needs %d or more)", JUR_NLOS); return JUR_ENLOS; }
  return JUR_OK;
}

/* ---- contributions of the emitters (formod TASK contrib) ------------------------------ */
/* Variant v of the atmosphere last set (the rows of m->h_atm, before the hydrostatic step) at `at` of rows `stride`
 * long: v < ng keeps q[v] and no other gas and no extinction, v == ng keeps the extinction and no gas; then the
 * hydrostatic step, as jur_model_set_atm would take it. */
static void pack_variant_rows(jur_model_t const *m, double *h, size_t stride, size_t at, int v) {
  int const n = (int)m->h_atm_n, ng = m->view.ng;
  size_t const nrow = 6 + (size_t)ng + m->view.nw;
  for (size_t row = 0; row < nrow; row++) {
    int const g = (int)row - 6, w = g - ng;
    double *const dst = h + row * stride + at;
    if ((g >= 0 && g < ng && g != v) || (w >= 0 && v < ng)) memset(dst, 0, sizeof(double) * n);
    else memcpy(dst, m->h_atm + row * (size_t)n, sizeof(double) * n);
  }
  hydrostatic_rows(m, h, stride, at, n);
}

/* With ctl->hydz >= 0 and H2O the emitter the hydrostatic step reads, zeroing q_H2O moves the pressure profile -- and
 * with it the line of sight -- of every variant but H2O's own.  Those naff variants are computed by their definition, as
 * kernel_ld does the Jacobian: the edited atmospheres stacked as profile slices (time stamps shifted by j * span), every
 * ray once per slice, one ordinary batched call; then the caller's atmosphere goes back on the device.  fb: device
 * scratch geom[7][N] | rad[N][nd] | tau[N][nd] | tp[3][N] (N = naff * nr) whose rad already holds the input radiances
 * once per slice (the NaN mask).  Waits for the stream. */
static int contrib_hydrostatic(jur_model_t *m, long nr, int naff, double const *d_geom, double *fb, int *d_status,
                               double *d_rad_c, double *d_tau_c, hipStream_t s) {
  int const ng = m->view.ng, nd = m->view.nd, n0 = (int)m->h_atm_n;
  size_t const nrow = 6 + (size_t)ng + m->view.nw, N = (size_t)naff * nr, NT = (size_t)naff * n0, nrd = (size_t)nr * nd;
  double *const fb_geom = fb, *const fb_rad = fb + 7 * N, *const fb_tau = fb_rad + N * nd, *const fb_tp = fb_tau + N * nd;
  double *const hg = (double *)malloc(sizeof(double) * 7 * ((size_t)nr + N));
  double *const h = (double *)malloc(sizeof(double) * nrow * NT);
  int rc = JUR_OK, moved = 0;
  hipError_t e = hipSuccess;
  if (!hg || !h) { rc = JUR_ENOMEM; goto done; }
  e = hipMemcpyAsync(hg, d_geom, sizeof(double) * 7 * (size_t)nr, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) goto done;
  {
    double *const g2 = hg + 7 * (size_t)nr;
    double tmin = m->h_atm[0], tmax = m->h_atm[0];
    for (int i = 0; i < n0; i++) { tmin = fmin(tmin, m->h_atm[i]); tmax = fmax(tmax, m->h_atm[i]); }
    for (long i = 0; i < nr; i++) { tmin = fmin(tmin, hg[i]); tmax = fmax(tmax, hg[i]); }
    double const span = (tmax - tmin) + 1.0;
    for (int v = 0, j = 0; v <= ng; v++) {
      if (v == m->view.ig_h2o) continue;          /* H2O's own variant came from the shared plane */
      pack_variant_rows(m, h, NT, (size_t)j * n0, v);
      stack_times(h + (size_t)j * n0, h + (size_t)j * n0, n0, (double)j * span);
      for (long i = 0; i < nr; i++)
        g2[(size_t)j * nr + i] = stacked_ray_time(m->h_atm, n0, hg[i], h + (size_t)j * n0, tmax + (naff + 1.0) * span);
      for (int k = 1; k < 7; k++)
        for (long i = 0; i < nr; i++) g2[k * N + (size_t)j * nr + i] = hg[k * (size_t)nr + i];
      j++;
    }
    e = hipMemcpyAsync(fb_geom, g2, sizeof(double) * 7 * N, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) goto done;
    m->h_atm_n = 0;                               /* the device no longer holds the caller's atmosphere */
    moved = 1;
    if ((rc = upload_atm_rows(m, h, (long)NT, JUR_ATM_PERTURBED))) goto done;
    if ((rc = jur_formod_device(m, (long)N, fb_geom, fb_rad, fb_tau, fb_tp, NULL, d_status ? d_status : m->d_status, s))) goto done;
    for (int v = 0, j = 0; v <= ng && e == hipSuccess; v++) {
      if (v == m->view.ig_h2o) continue;
      e = hipMemcpyAsync(d_rad_c + (size_t)v * nrd, fb_rad + (size_t)j * nrd, sizeof(double) * nrd, hipMemcpyDeviceToDevice, s);
      if (e == hipSuccess) e = hipMemcpyAsync(d_tau_c + (size_t)v * nrd, fb_tau + (size_t)j * nrd, sizeof(double) * nrd, hipMemcpyDeviceToDevice, s);
      j++;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
  }
done:
  if (e != hipSuccess && !rc) { jur_set_error("formod_contrib: %s", hipGetErrorString(e)); rc = JUR_EHIP; }
  if (moved && h) {                               /* the caller's atmosphere back, hydrostatic step and all */
    memcpy(h, m->h_atm, sizeof(double) * nrow * n0);
    hydrostatic_rows(m, h, (size_t)n0, 0, n0);
    int const r2 = upload_atm_rows(m, h, n0, JUR_ATM_CALLER);
    if (!r2) m->h_atm_n = n0;
    else m->view.atm_np = 0;                      /* never the stacked one: the next call is refused ("no atmosphere set") */
    if (!rc) rc = r2;
  }
  free(hg);
  free(h);
  return rc;
}

int jur_formod_contrib_device(jur_model_t *m, long nr, double const *d_geom, double *d_rad, double *d_tau, double *d_tp, int *d_np,
                              int *d_status, double *d_rad_c, double *d_tau_c, void *stream) {
  if (!m || nr < 0 || (nr > 0 && (!d_geom || !d_rad || !d_tau || !d_tp || !d_rad_c || !d_tau_c))) {
    jur_set_error("formod_contrib_device: bad arguments");
    return JUR_EINVAL;
  }
  if (nr == 0) return JUR_OK;
  if (m->view.atm_np < 2) { jur_set_error("formod_contrib_device: no atmosphere set"); return JUR_EINVAL; }
  HIPCHK(hipSetDevice(m->device));
  hipStream_t const s = (hipStream_t)stream;
  int const nd = m->view.nd;
  /* the variants whose line of sight is not the call's: all but H2O's when the hydrostatic step reads q_H2O */
  int const naff = (m->ctl->hydz >= 0 && m->view.ig_h2o >= 0) ? m->view.ng : 0;
  size_t const nrd = (size_t)nr * nd, N = (size_t)naff * nr;
  double *fb = NULL;
  if (naff) {
    if (!m->h_atm || m->h_atm_n != m->view.atm_np) {
      jur_set_error("formod_contrib_device: with HYDZ >= 0 the atmosphere must have been set by jur_model_set_atm");
      return JUR_EINVAL;
    }
    HIPCHK(hipMalloc((void **)&fb, sizeof(double) * N * (10 + 2 * (size_t)nd)));
    hipError_t e = hipSuccess;
    for (int j = 0; j < naff && e == hipSuccess; j++)    /* the NaN mask, before the radiance update overwrites it */
      e = hipMemcpyAsync(fb + 7 * N + (size_t)j * nrd, d_rad, sizeof(double) * nrd, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) { (void)hipFree(fb); jur_set_error("formod_contrib_device: %s", hipGetErrorString(e)); return JUR_EHIP; }
  }
  contrib_out_t const co = {d_rad_c, d_tau_c};
  int rc = formod_device_body(m, nr, d_geom, nr, d_rad, d_tau, d_tp, nr, d_np, d_status, stream, &co);
  if (!rc && naff) rc = contrib_hydrostatic(m, nr, naff, d_geom, fb, d_status, d_rad_c, d_tau_c, s);
  if (fb) {
    (void)hipStreamSynchronize(s);
    (void)hipFree(fb);
  }
  return rc;
}

int jur_formod_contrib_host(jur_model_t *m, long nr, double const *const geom[7], double *rad, double *tau, double *const tp[3],
                            int *np_out, double *rad_c, double *tau_c) {
  if (!m || nr < 0 || !rad_c || !tau_c) { jur_set_error("formod_contrib_host: bad arguments"); return JUR_EINVAL; }
  if (nr == 0) return JUR_OK;
  HIPCHK(hipSetDevice(m->device));
  int const nd = m->view.nd;
  size_t const N = (size_t)nr, nrd = N * nd, nc = (size_t)(m->view.ng + 1) * nrd;
  hipStream_t const s = m->stream;
  int rc = wait_done(m, s);
  if (!rc) rc = ensure_io(m, nr, 1);
  if (rc) return rc;
  if ((long)(2 * nc) > m->ctb_cap) {
    if (m->d_ctb) (void)hipFree(m->d_ctb);
    m->d_ctb = NULL; m->ctb_cap = 0;
    HIPCHK(hipMalloc((void **)&m->d_ctb, sizeof(double) * 2 * nc));
    m->ctb_cap = (long)(2 * nc);
  }
  /* the staging of jur_formod_host's packages: the model's pinned image, one transfer in, one out */
  double *const d_geom = m->d_io, *const d_rad = d_geom + 7 * N, *const d_tau = d_rad + nrd, *const d_tp = d_tau + nrd;
  double *const h_geom = m->h_io, *const h_rad = h_geom + 7 * N, *const h_tau = h_rad + nrd, *const h_tp = h_tau + nrd;
  int *const h_np = (int *)(h_tp + 3 * N);
  for (int k = 0; k < 7; k++) par_memcpy(h_geom + k * N, geom[k], sizeof(double) * N);
  par_memcpy(h_rad, rad, sizeof(double) * nrd);
  HIPCHK(hipMemcpyAsync(d_geom, h_geom, sizeof(double) * (7 * N + nrd), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(m->d_status, 0, sizeof(int), s));
  if ((rc = jur_formod_contrib_device(m, nr, d_geom, d_rad, d_tau, d_tp, m->d_io_np, m->d_status, m->d_ctb, m->d_ctb + nc, s)))
    return rc;
  HIPCHK(hipMemcpyAsync(h_rad, d_rad, sizeof(double) * (2 * nrd + 3 * N), hipMemcpyDeviceToHost, s));
  if (np_out) HIPCHK(hipMemcpyAsync(h_np, m->d_io_np, sizeof(int) * N, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(m->h_status, m->d_status, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(rad_c, m->d_ctb, sizeof(double) * nc, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(tau_c, m->d_ctb + nc, sizeof(double) * nc, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (*m->h_status & 1) { jur_set_error("Too many LOS points! (a ray needs %d or more)", JUR_NLOS); return JUR_ENLOS; }
  par_memcpy(rad, h_rad, sizeof(double) * nrd);
  par_memcpy(tau, h_tau, sizeof(double) * nrd);
  for (int k = 0; k < 3; k++) memcpy(tp[k], h_tp + k * N, sizeof(double) * N);
  if (np_out) memcpy(np_out, h_np, sizeof(int) * N);
  return JUR_OK;
}

/* ---- Curtis-Godson columns ------------------------------------------------------ */
/* Traces the rays and returns, per ray, gas and LOS point, the Curtis-Godson pressure, temperature and
 * cumulative column (curtis_godson, jr_common.h:455-473).  cgp/cgt/cgu are host arrays
 * [nr][ng][JUR_NLOS] (points at and beyond np[ray] are 0); tp/np_out as in jur_formod_host. */
int jur_curtis_godson_host(jur_model_t *m, long nr, double const *const geom[7], double *cgp, double *cgt, double *cgu,
                           double *const tp[3], int *np_out) {
  if (!m || nr < 1 || !cgp || !cgt || !cgu) { jur_set_error("curtis_godson: bad arguments"); return JUR_EINVAL; }
  if (m->view.atm_np < 2) { jur_set_error("curtis_godson: no atmosphere set"); return JUR_EINVAL; }
  view_set_k_zero(m);
  HIPCHK(hipSetDevice(m->device));
  int const ng = m->view.ng;
  int rc = ensure_workspace(m, nr);
  if (rc) return rc;
  long const Rt = m->use_trace_rays;
  hipStream_t s = m->stream;
  if ((rc = wait_done(m, s))) return rc;
  size_t const per_ray = (size_t)(ng > 0 ? ng : 1) * JUR_NLOS;
  double *d_geom = NULL, *d_out = NULL, *d_tp = NULL;
  int *d_np = NULL;
  hipError_t e = hipMalloc((void **)&d_geom, sizeof(double) * 7 * (size_t)nr);
  if (e == hipSuccess) e = hipMalloc((void **)&d_tp, sizeof(double) * 3 * (size_t)nr);
  if (e == hipSuccess) e = hipMalloc((void **)&d_np, sizeof(int) * (size_t)nr);
  if (e == hipSuccess) e = hipMalloc((void **)&d_out, sizeof(double) * 3 * per_ray * (size_t)nr);
  if (e != hipSuccess) { rc = JUR_EHIP; jur_set_error("curtis_godson: hipMalloc failed"); goto done; }
  for (int k = 0; k < 7; k++)
    if (hipMemcpyAsync(d_geom + (size_t)k * nr, geom[k], sizeof(double) * nr, hipMemcpyHostToDevice, s) != hipSuccess) { rc = JUR_EHIP; goto done; }
  if (hipMemsetAsync(m->d_status, 0, sizeof(int), s) != hipSuccess) { rc = JUR_EHIP; goto done; }
  {
    double *d_cgp = d_out, *d_cgt = d_out + per_ray * (size_t)nr, *d_cgu = d_out + 2 * per_ray * (size_t)nr;
    for (long t0 = 0; t0 < nr; t0 += Rt) {
      jur_chunk_t c;
      memset(&c, 0, sizeof c);
      c.n = (int)((nr - t0 < Rt) ? nr - t0 : Rt);
      c.stride = (int)Rt;
      c.stride_eps = (int)m->use_rays;
      c.first = t0;
      c.order = NULL;
      for (int k = 0; k < 7; k++) c.geom[k] = d_geom + (size_t)k * nr;
      for (int k = 0; k < 3; k++) c.tp[k] = d_tp + (size_t)k * nr;
      c.np_out = d_np;
      c.np = m->d_np;
      c.tsurf = m->d_tsurf;
      c.los = m->d_los;
      c.eps = m->d_eps;
      c.status = m->d_status;
      int ek = jurk_launch_trace(&m->view, &m->track, &m->cloud, &c, s);
      if (!ek) ek = jurk_launch_cg(&m->view, &c, d_cgp, d_cgt, d_cgu, s);
      if (ek) { jur_set_error("curtis_godson: kernel launch failed: %s", hipGetErrorString((hipError_t)ek)); rc = JUR_EHIP; goto done; }
    }
    int status = 0;
    hipError_t ec = hipMemcpyAsync(cgp, d_cgp, sizeof(double) * per_ray * (size_t)nr, hipMemcpyDeviceToHost, s);
    if (ec == hipSuccess) ec = hipMemcpyAsync(cgt, d_cgt, sizeof(double) * per_ray * (size_t)nr, hipMemcpyDeviceToHost, s);
    if (ec == hipSuccess) ec = hipMemcpyAsync(cgu, d_cgu, sizeof(double) * per_ray * (size_t)nr, hipMemcpyDeviceToHost, s);
    for (int k = 0; k < 3 && tp && ec == hipSuccess; k++)
      ec = hipMemcpyAsync(tp[k], d_tp + (size_t)k * nr, sizeof(double) * nr, hipMemcpyDeviceToHost, s);
    if (np_out && ec == hipSuccess) ec = hipMemcpyAsync(np_out, d_np, sizeof(int) * nr, hipMemcpyDeviceToHost, s);
    if (ec == hipSuccess) ec = hipMemcpyAsync(&status, m->d_status, sizeof(int), hipMemcpyDeviceToHost, s);
    if (ec == hipSuccess) ec = hipStreamSynchronize(s);
    if (ec != hipSuccess) { jur_set_error("curtis_godson: copy back failed: %s", hipGetErrorString(ec)); rc = JUR_EHIP; goto done; }
    if (status & 1) { jur_set_error("Too many LOS points! (a ray needs %d or more)", JUR_NLOS); rc = JUR_ENLOS; }
  }
done:
  if (d_geom) (void)hipFree(d_geom);
  if (d_tp) (void)hipFree(d_tp);
  if (d_np) (void)hipFree(d_np);
  if (d_out) (void)hipFree(d_out);
  return rc;
}

/* ---- field-of-view convolution of results that stay on the device ------------------- */
int jur_fov_apply_device(jur_model_t *m, long nr, double const *d_time, double const *d_vpz, double *d_rad, double *d_tau,
                         int n, double const *dz, double const *w, void *stream) {
  if (!m || nr < 1 || n < 1 || n > JUR_NSHAPE || !d_time || !d_vpz || !d_rad || !d_tau || !dz || !w) {
    jur_set_error("jur_fov_apply_device: bad arguments");
    return JUR_EINVAL;
  }
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  int const nd = m->view.nd;
  size_t const vals = (size_t)nr * nd;
  /* scratch kept by the model and only ever grown: rad0 | tau0 | dz | w | status word.  Every ray reads the
   * UNconvolved neighbours; the status word is this path's own (a forward-model call in flight on another stream
   * keeps m->d_status to itself), and nothing here allocates or frees per call (hipFree would wait for the whole
   * device). */
  long const need = (long)(2 * vals + 2 * (size_t)JUR_NSHAPE + 1);
  if (need > m->fov_cap) {
    if (m->d_fov) (void)hipFree(m->d_fov);
    m->d_fov = NULL; m->fov_cap = 0;
    HIPCHK(hipMalloc((void **)&m->d_fov, sizeof(double) * (size_t)need));
    m->fov_cap = need;
  }
  double *const tmp = m->d_fov;
  int *const d_st = (int *)(tmp + 2 * vals + 2 * (size_t)JUR_NSHAPE);
  int *const h_st = m->h_status + 1;             /* second word of the pinned status block */
  int rc = JUR_OK, status = 0;
  hipError_t e = hipMemcpyAsync(tmp, d_rad, sizeof(double) * vals, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(tmp + vals, d_tau, sizeof(double) * vals, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(tmp + 2 * vals, dz, sizeof(double) * n, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(tmp + 2 * vals + JUR_NSHAPE, w, sizeof(double) * n, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(d_st, 0, sizeof(int), s);
  if (e == hipSuccess)
    e = (hipError_t)jurk_launch_fov(nr, nd, d_time, d_vpz, tmp, tmp + vals, d_rad, d_tau, nd, n, tmp + 2 * vals,
                                    tmp + 2 * vals + JUR_NSHAPE, d_st, s);
  if (e == hipSuccess) e = hipMemcpyAsync(h_st, d_st, sizeof(int), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { jur_set_error("jur_fov_apply_device: %s", hipGetErrorString(e)); rc = JUR_EHIP; }
  else status = *h_st;
  if (!rc && (status & 2)) { jur_set_error("Cannot apply FOV convolution!"); rc = JUR_EINVAL; }
  return rc;
}

/* ---- field of view of the scene entries ---------------------------------------------- */
int jur_model_set_fov(jur_model_t *m, int n, double const *dz, double const *w) {
  char const *const who = "jur_model_set_fov";
  if (!m) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  if (n < 0 || n > JUR_NSHAPE) { jur_set_error("%s: n = %d: 0 (off) to %d points", who, n, JUR_NSHAPE); return JUR_EINVAL; }
  if (n == 0) { m->fov_n = 0; return JUR_OK; }
  if (!dz || !w) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  double wsum = 0;
  for (int k = 0; k < n; k++) {
    if (!isfinite(dz[k]) || !isfinite(w[k])) {
      jur_set_error("%s: point %d of the shape is (%g, %g): not finite", who, k, dz[k], w[k]);
      return JUR_EINVAL;
    }
    wsum += w[k];
  }
  if (!isfinite(wsum) || wsum == 0) { jur_set_error("%s: the weights sum to %g: 0 or not finite", who, wsum); return JUR_EINVAL; }
  HIPCHK(hipSetDevice(m->device));
  if (!m->fov_shape && !(m->fov_shape = (double *)calloc(2 * (size_t)JUR_NSHAPE, sizeof(double)))) {
    jur_set_error("%s: out of memory", who);
    return JUR_ENOMEM;
  }
  if (!m->d_fov_shape) HIPCHK(hipMalloc((void **)&m->d_fov_shape, sizeof(double) * 2 * (size_t)JUR_NSHAPE));
  /* (a scene entry waits for its stream before it returns: nothing reads the old shape any more) */
  m->fov_n = 0;
  memcpy(m->fov_shape, dz, sizeof(double) * (size_t)n);
  memcpy(m->fov_shape + JUR_NSHAPE, w, sizeof(double) * (size_t)n);
  HIPCHK(hipMemcpy(m->d_fov_shape, m->fov_shape, sizeof(double) * 2 * (size_t)JUR_NSHAPE, hipMemcpyHostToDevice));
  m->fov_n = n;
  return JUR_OK;
}

int jur_model_fov(jur_model_t const *m, int *n, double *dz, double *w) {
  if (!m || !n) { jur_set_error("jur_model_fov: null argument"); return JUR_EINVAL; }
  *n = m->fov_n;
  if (dz && m->fov_n) memcpy(dz, m->fov_shape, sizeof(double) * (size_t)m->fov_n);
  if (w && m->fov_n) memcpy(w, m->fov_shape + JUR_NSHAPE, sizeof(double) * (size_t)m->fov_n);
  return JUR_OK;
}

/* ---- hydrostatic balance of the scene entries, slice by slice ------------------------------ */
int jur_model_set_scene_hydz(jur_model_t *m, double hydz) {
  char const *const who = "jur_model_set_scene_hydz";
  if (!m) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  if (!(hydz - hydz == 0)) { jur_set_error("%s: hydz is %g: not finite (a negative value switches the balance off)", who, hydz); return JUR_EINVAL; }
  double const v = hydz >= 0 ? hydz : -1;
  /* what set_atm last uploaded was uploaded under the old setting: never taken for current under the new one */
  if (v != m->scene_hydz) m->h_atm_n = 0;
  m->scene_hydz = v;
  return JUR_OK;
}

double jur_model_scene_hydz(jur_model_t const *m) { return m ? m->scene_hydz : -1; }

/* the box on the state: held by value, expanded per element by the entries that move a state when a call starts */
int jur_model_set_state_bounds(jur_model_t *m, int nq, double const *lo, double const *hi) {
  char const *const who = "jur_model_set_state_bounds";
  if (!m) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  if (nq == 0 || !lo || !hi) { m->sb_nq = 0; return JUR_OK; }
  int const rc = jur_state_bounds_check(who, m->view.ng, m->view.nw, nq, lo, hi);
  if (rc) return rc;                                /* (what was set before stays set) */
  memcpy(m->sb_lo, lo, sizeof(double) * (size_t)nq);
  memcpy(m->sb_hi, hi, sizeof(double) * (size_t)nq);
  m->sb_nq = nq;
  return JUR_OK;
}

int jur_model_state_bounds(jur_model_t const *m, double *lo, double *hi) {
  if (!m) return 0;
  if (lo) memcpy(lo, m->sb_lo, sizeof(double) * (size_t)m->sb_nq);
  if (hi) memcpy(hi, m->sb_hi, sizeof(double) * (size_t)m->sb_nq);
  return m->sb_nq;
}

/* ---- the Jacobian of the retrieval loop, reused between iterations ------------------------- */
int jur_model_set_kernel_recomp(jur_model_t *m, int every) {
  char const *const who = "jur_model_set_kernel_recomp";
  if (!m) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  if (every < 1) { jur_set_error("%s: every is %d: the Jacobian is recomputed every n-th iteration, n >= 1", who, every); return JUR_EINVAL; }
  m->kernel_recomp = every;
  return JUR_OK;
}

int jur_model_kernel_recomp(jur_model_t const *m) { return m ? m->kernel_recomp : 1; }

/* ---- untraceable rays in jur_trial_scene_host and jur_retrieve_scene_host ------------------ */
int jur_model_set_scene_overflow(jur_model_t *m, int mode) {
  char const *const who = "jur_model_set_scene_overflow";
  if (!m) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  if (mode != JUR_OVERFLOW_ERROR && mode != JUR_OVERFLOW_ISOLATE) {
    jur_set_error("%s: unknown mode %d: JUR_OVERFLOW_ERROR (%d) or JUR_OVERFLOW_ISOLATE (%d)", who, mode, JUR_OVERFLOW_ERROR, JUR_OVERFLOW_ISOLATE);
    return JUR_EINVAL;
  }
  m->scene_overflow = mode;
  return JUR_OK;
}

int jur_model_scene_overflow(jur_model_t const *m) { return m ? m->scene_overflow : JUR_OVERFLOW_ERROR; }

int jur_model_last_scene_overflow(jur_model_t const *m, long *trial_cells, long *failed_slices) {
  if (!m) { jur_set_error("jur_model_last_scene_overflow: null argument"); return JUR_EINVAL; }
  if (trial_cells) *trial_cells = m->ov_cells;
  if (failed_slices) *failed_slices = m->ov_failed;
  return JUR_OK;
}

/* The retrieval windows live in the model's copy of the control block and nowhere else: every entry that derives a state
 * reads them there when it is called (jur_scene_layout, jur_scene_slices, jur_state_vector), and neither the view, the
 * uploaded atmosphere nor the tables were made from them. */
static void ret_windows_copy(ctl_t *to, ctl_t const *from, int ng, int nw) {
  to->retp_zmin = from->retp_zmin; to->retp_zmax = from->retp_zmax;
  to->rett_zmin = from->rett_zmin; to->rett_zmax = from->rett_zmax;
  for (int g = 0; g < ng; g++) { to->retq_zmin[g] = from->retq_zmin[g]; to->retq_zmax[g] = from->retq_zmax[g]; }
  for (int w = 0; w < nw; w++) { to->retk_zmin[w] = from->retk_zmin[w]; to->retk_zmax[w] = from->retk_zmax[w]; }
}

static int ret_windows_check(char const *who, int ng, int nw, ctl_t const *ctl) {
  if (ctl->retp_zmin != ctl->retp_zmin || ctl->retp_zmax != ctl->retp_zmax) { jur_set_error("%s: the window of p is NaN", who); return JUR_EINVAL; }
  if (ctl->rett_zmin != ctl->rett_zmin || ctl->rett_zmax != ctl->rett_zmax) { jur_set_error("%s: the window of T is NaN", who); return JUR_EINVAL; }
  for (int g = 0; g < ng; g++)
    if (ctl->retq_zmin[g] != ctl->retq_zmin[g] || ctl->retq_zmax[g] != ctl->retq_zmax[g]) { jur_set_error("%s: the window of gas %d is NaN", who, g); return JUR_EINVAL; }
  for (int w = 0; w < nw; w++)
    if (ctl->retk_zmin[w] != ctl->retk_zmin[w] || ctl->retk_zmax[w] != ctl->retk_zmax[w]) { jur_set_error("%s: the window of extinction %d is NaN", who, w); return JUR_EINVAL; }
  return JUR_OK;
}

int jur_model_set_ret_windows(jur_model_t *m, ctl_t const *ctl) {
  char const *const who = "jur_model_set_ret_windows";
  if (!m || !ctl) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  int const ng = m->view.ng, nw = m->view.nw;
  int const rc = ret_windows_check(who, ng, nw, ctl);
  if (rc) return rc;
  ret_windows_copy(m->ctl, ctl, ng, nw);              /* (after every check: what was set stays set on a refusal) */
  return JUR_OK;
}

int jur_model_ret_windows(jur_model_t const *m, ctl_t *ctl) {
  if (!m || !ctl) { jur_set_error("jur_model_ret_windows: null argument"); return JUR_EINVAL; }
  ret_windows_copy(ctl, m->ctl, m->view.ng, m->view.nw);
  return JUR_OK;
}

/* Events around the kernels of jur_kernel_scene_host while timing is on (kind 5) */
static int scene_timed_begin(jur_model_t *m, hipStream_t s) {
  int const ti = (m->timing && m->ntimed < JUR_MAX_TIMED) ? m->ntimed++ : -1;
  if (ti >= 0) { m->evkind[ti] = 5; if (hipEventRecord(m->evpool[2 * ti], s) != hipSuccess) (void)hipGetLastError(); }
  return ti;
}
static void scene_timed_end(jur_model_t *m, int ti, hipStream_t s) {
  if (ti >= 0 && hipEventRecord(m->evpool[2 * ti + 1], s) != hipSuccess) (void)hipGetLastError();
}
/* one launch between the two records: yields the launch's status */
#define SCENE_TIMED(m, s, launch) __extension__ ({ int const ti_ = scene_timed_begin(m, s); int const ek_ = (launch); scene_timed_end(m, ti_, s); ek_; })
/* fmt: "%s: <what> kernel launch failed" */
static int launch_failed(char const *fmt, char const *who) { jur_set_error(fmt, who); return JUR_EHIP; }

/* jur_scene_hydro_kernel on the segments hy (device) of rows [nrow][ld] as the model lays an atmosphere out:
 * time, z, lon, lat, p, T, q[ng], k[nw].  Timed with the scene entries' kernels. */
static int scene_hydro_launch(jur_model_t *m, hipStream_t s, jur_hyseg_t hy, double *rows, size_t ld) {
  if (hy.n <= 0) return 0;
  int const ig = m->view.ig_h2o;
  jur_scene_hydro_t hq;
  memset(&hq, 0, sizeof hq);
  hq.nseg = hy.n; hq.at = hy.at; hq.len = hy.len; hq.hydz = m->scene_hydz;
  hq.z = rows + 1 * ld; hq.lat = rows + 3 * ld; hq.p = rows + 4 * ld; hq.t = rows + 5 * ld;
  hq.q = ig >= 0 ? rows + (6 + (size_t)ig) * ld : NULL;
  return SCENE_TIMED(m, s, jurk_scene_hydro(&hq, s));
}

/* ---- full a-priori precision of the slices ------------------------------------------------ */
static void prior_precision_drop(jur_model_t *m) {
  m->pp_nslice = 0;
  if (m->d_pp) (void)hipFree(m->d_pp);
  m->d_pp = NULL;
  free(m->pp_wptr); m->pp_wptr = NULL;
  free(m->pp_R); m->pp_R = NULL;
}

int jur_model_set_prior_precision(jur_model_t *m, long nslice, long const *wptr, double const *R) {
  char const *const who = "jur_model_set_prior_precision";
  if (!m || nslice < 0) { jur_set_error("%s: bad arguments", who); return JUR_EINVAL; }
  HIPCHK(hipSetDevice(m->device));
  /* (a scene entry waits for its stream before it returns: nothing reads the old matrices any more) */
  if (nslice == 0 || !R) { prior_precision_drop(m); return JUR_OK; }
  if (nslice > 0x7fffffffL) { jur_set_error("%s: at most 2^31-1 slices", who); return JUR_EINVAL; }
  if (!wptr) { jur_set_error("%s: null argument (wptr)", who); return JUR_EINVAL; }
  int rc = jur_prior_check_R(who, nslice, wptr, R);
  if (rc) return rc;                                       /* (what was set stays set) */
  size_t const NS = (size_t)nslice;
  long *ptr = (long *)malloc(sizeof(long) * 2 * (NS + 1));
  if (!ptr) { jur_set_error("%s: out of memory", who); return JUR_ENOMEM; }
  long *const aptr = ptr + NS + 1;
  memcpy(ptr, wptr, sizeof(long) * (NS + 1));
  aptr[0] = 0;
  for (long q = 0; q < nslice; q++) { long const w = wptr[q + 1] - wptr[q]; aptr[q + 1] = aptr[q] + w * w; }
  size_t const NA = (size_t)aptr[nslice];
  double *hR = (double *)malloc(sizeof(double) * (NA ? NA : 1));
  void *d = NULL;
  if (!hR) { free(ptr); jur_set_error("%s: out of memory", who); return JUR_ENOMEM; }
  memcpy(hR, R, sizeof(double) * NA);
  if (hipMalloc(&d, sizeof(long) * 2 * (NS + 1) + sizeof(double) * (NA ? NA : 1)) != hipSuccess) {
    (void)hipGetLastError(); free(ptr); free(hR);
    jur_set_error("%s: no device memory for %zu bytes", who, sizeof(long) * 2 * (NS + 1) + sizeof(double) * NA);
    return JUR_ENOMEM;
  }
  hipError_t e = hipMemcpy(d, ptr, sizeof(long) * 2 * (NS + 1), hipMemcpyHostToDevice);
  if (NA && e == hipSuccess) e = hipMemcpy((long *)d + 2 * (NS + 1), hR, sizeof(double) * NA, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d); free(ptr); free(hR);
    jur_set_error("%s: %s", who, hipGetErrorString(e));
    return JUR_EHIP;
  }
  prior_precision_drop(m);
  m->pp_wptr = ptr; m->pp_R = hR; m->d_pp = d; m->pp_nslice = nslice;
  return JUR_OK;
}

long jur_model_prior_precision(jur_model_t const *m, long *wptr, double *R) {
  if (!m) { jur_set_error("jur_model_prior_precision: null argument"); return JUR_EINVAL; }
  if (m->pp_nslice == 0) return 0;
  size_t const NS = (size_t)m->pp_nslice;
  if (wptr) memcpy(wptr, m->pp_wptr, sizeof(long) * (NS + 1));
  if (R) memcpy(R, m->pp_R, sizeof(double) * (size_t)m->pp_wptr[2 * NS + 1]);
  return m->pp_nslice;
}

/* the device's R of the model for a call laid out by (nslice, wptr), NULL where none is set; JUR_EINVAL for another layout
 * or a missing prior_ivar */
static int prior_precision_for(jur_model_t const *m, char const *who, long nslice, long const *wptr, int have_ivar,
                               double const **d_R) {
  *d_R = NULL;
  if (m->pp_nslice == 0) return JUR_OK;
  int const rc = jur_prior_check_layout(who, m->pp_nslice, m->pp_wptr, nslice, wptr);
  if (rc) return rc;
  if (!have_ivar) {
    jur_set_error("%s: a prior precision is set in the model: prior_ivar (it may be all zeros) and its partner are required", who);
    return JUR_EINVAL;
  }
  *d_R = (double const *)((long const *)m->d_pp + 2 * ((size_t)nslice + 1));
  return JUR_OK;
}

/* The scene entries' part of the convolution.  The buffer the convolved radiances of a pass go to (nval doubles, the
 * model's grow-only scratch of jur_fov_apply_device, which holds nothing between calls) ... */
static int scene_fov_reserve(jur_model_t *m, size_t nval) {
  if ((long)nval > m->fov_cap) {
    if (m->d_fov) (void)hipFree(m->d_fov);
    m->d_fov = NULL; m->fov_cap = 0;
    HIPCHK(hipMalloc((void **)&m->d_fov, sizeof(double) * nval));
    m->fov_cap = (long)nval;
  }
  return JUR_OK;
}

/* ... and the effective mask of the call as the doubles the kernels test: +0.0 where live, NaN elsewhere (malloc'ed);
 * what jur_scene_fov_live refuses is refused in the entry's name */
static int scene_fov_mask(char const *who, int nd, long nr, double const *time, double const *rad_in, double **out) {
  size_t const n = (size_t)nr * (size_t)nd;
  unsigned char *live = (unsigned char *)malloc(n ? n : 1);
  double *mask = (double *)malloc(sizeof(double) * (n ? n : 1));
  *out = NULL;
  if (!live || !mask) { free(live); free(mask); jur_set_error("%s: out of memory", who); return JUR_ENOMEM; }
  long const rc = jur_scene_fov_live(nd, nr, time, rad_in, live);
  if (rc < 0) {
    char msg[400];
    snprintf(msg, sizeof msg, "%s", jur_last_error());
    jur_set_error("%s: %s", who, msg);
    free(live); free(mask);
    return (int)rc;
  }
  for (size_t i = 0; i < n; i++) mask[i] = live[i] ? 0. : NAN;
  free(live);
  *out = mask;
  return JUR_OK;
}

/* The device slab of the scene entries (grow-only; it holds nothing between calls): selects the device, waits for the
 * model's earlier calls, as every entry does, and leaves at least `bytes` in m->d_scene; *stream: the model's */
static int scene_slab_reserve(jur_model_t *m, char const *who, size_t bytes, hipStream_t *stream) {
  if (hipSetDevice(m->device) != hipSuccess) { jur_set_error("%s: cannot select the device", who); return JUR_EHIP; }
  *stream = m->stream;
  int const rc = wait_done(m, m->stream);
  if (rc) return rc;
  if (bytes > m->scene_bytes) {
    if (m->d_scene) (void)hipFree(m->d_scene);
    m->d_scene = NULL; m->scene_bytes = 0;
    if (hipMalloc(&m->d_scene, bytes) != hipSuccess) {
      (void)hipGetLastError(); jur_set_error("%s: no device memory for %zu bytes", who, bytes); return JUR_ENOMEM;
    }
    m->scene_bytes = bytes;
  }
  return JUR_OK;
}

/* one more part of the slab: does it fit beside the *used bytes in the half of the workspace budget the slab may take?
 * (sums in double, term by term in the order the parts join); where it does it is counted */
static int scene_fits(jur_model_t const *m, double *used, size_t add) {
  if (*used + (double)add > (double)(m->ws_budget / 2)) return 0;
  *used += (double)add;
  return 1;
}

/* what the status word that has come home (m->h_status) says of the forward models of a scene entry; isolate: the
 * entry deals with untraceable rays itself (JUR_OVERFLOW_ISOLATE) and bit 1 does not end it */
static int scene_status_rc(jur_model_t const *m, char const *who, int isolate) {
  if ((*m->h_status & 1) && !isolate) { jur_set_error("Too many LOS points! (a ray needs %d or more)", JUR_NLOS); return JUR_ENLOS; }
  if (*m->h_status & 2) { jur_set_error("%s: Cannot apply FOV convolution!", who); return JUR_EINVAL; }
  return JUR_OK;
}

/* ---- known-answer hooks ----------------------------------------------------------- */
/* nin input arrays and nout in/out arrays of n doubles each go to the device as one slab [nin + nout][n] */
static int kat_slab(jur_model_t *m, long n, int nin, double const *const in[], int nout, double *const out[], double **d) {
  *d = NULL;
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipMalloc((void **)d, sizeof(double) * (size_t)n * (size_t)(nin + nout)));
  for (int k = 0; k < nin; k++) HIPCHK(hipMemcpy(*d + (size_t)k * n, in[k], sizeof(double) * n, hipMemcpyHostToDevice));
  for (int k = 0; k < nout; k++) HIPCHK(hipMemcpy(*d + (size_t)(nin + k) * n, out[k], sizeof(double) * n, hipMemcpyHostToDevice));
  return JUR_OK;
}

static int kat_finish(jur_model_t *m, int ek, long n, int nin, int nout, double *const out[], double *d) {
  int rc = JUR_OK;
  if (ek) { jur_set_error("known-answer kernel not launched: %s", hipGetErrorString((hipError_t)ek)); rc = (ek == (int)hipErrorInvalidValue) ? JUR_EINVAL : JUR_EHIP; }
  if (!rc && hipStreamSynchronize(m->stream) != hipSuccess) { jur_set_error("known-answer kernel failed"); rc = JUR_EHIP; }
  for (int k = 0; k < nout && !rc; k++)
    if (hipMemcpy(out[k], d + (size_t)(nin + k) * n, sizeof(double) * n, hipMemcpyDeviceToHost) != hipSuccess) rc = JUR_EHIP;
  if (d) (void)hipFree(d);
  return rc;
}

int jur_kat_ega_eps(jur_model_t *m, int ig, int id, long n, double const *tau, double const *t, double const *u,
                    double const *p, int mode, int chain, double *out) {
  if (!m || n < 1 || ig < 0 || ig >= m->view.ng || id < 0 || id >= m->view.nd) { jur_set_error("kat_ega_eps: bad arguments"); return JUR_EINVAL; }
  double const *in[4] = {tau, t, u, p};
  double *io[1] = {out}, *d;
  int rc = kat_slab(m, n, 4, in, 1, io, &d);
  if (rc) { if (d) (void)hipFree(d); return rc; }
  int const ek = jurk_kat_ega(&m->view, ig, id, n, d, d + n, d + 2 * n, d + 3 * n, mode, chain, d + 4 * n, m->stream);
  return kat_finish(m, ek, n, 4, 1, io, d);
}

int jur_kat_cga_eps(jur_model_t *m, int ig, int id, long n, double const *tau, double const *cgt, double const *cgu,
                    double const *cgp, int mode, int chain, double *out) {
  if (!m || n < 1 || ig < 0 || ig >= m->view.ng || id < 0 || id >= m->view.nd) { jur_set_error("kat_cga_eps: bad arguments"); return JUR_EINVAL; }
  double const *in[4] = {tau, cgt, cgu, cgp};
  double *io[1] = {out}, *d;
  int rc = kat_slab(m, n, 4, in, 1, io, &d);
  if (rc) { if (d) (void)hipFree(d); return rc; }
  int const ek = jurk_kat_cga(&m->view, ig, id, n, d, d + n, d + 2 * n, d + 3 * n, mode, chain, d + 4 * n, m->stream);
  return kat_finish(m, ek, n, 4, 1, io, d);
}

int jur_kat_continua(jur_model_t *m, int id, long n, double const *p, double const *t, double const *q, double const *u_co2,
                     double const *u_h2o, double *out) {
  if (!m || n < 1 || id < 0 || id >= m->view.nd) { jur_set_error("kat_continua: bad arguments"); return JUR_EINVAL; }
  double const *in[5] = {p, t, q, u_co2, u_h2o};
  double *io[4] = {out, out + n, out + 2 * n, out + 3 * n}, *d;
  int rc = kat_slab(m, n, 5, in, 4, io, &d);
  if (rc) { if (d) (void)hipFree(d); return rc; }
  int const ek = jurk_kat_continua(&m->view, id, n, d, d + n, d + 2 * n, d + 3 * n, d + 4 * n, d + 5 * n, m->stream);
  return kat_finish(m, ek, n, 5, 4, io, d);
}

int jur_kat_update(jur_model_t *m, int id, long n, int what, double const *a, double const *b, double const *c, double *rad,
                   double *tau, double *src) {
  if (!m || n < 1 || id < 0 || id >= m->view.nd || (what != 0 && what != 1)) { jur_set_error("kat_update: bad arguments"); return JUR_EINVAL; }
  double const *in[3] = {a, b, c};
  double *io[3] = {rad, tau, src}, *d;
  int rc = kat_slab(m, n, 3, in, 3, io, &d);
  if (rc) { if (d) (void)hipFree(d); return rc; }
  int const ek = jurk_kat_update(&m->view, id, n, what, d, d + n, d + 2 * n, d + 3 * n, d + 4 * n, d + 5 * n, m->stream);
  return kat_finish(m, ek, n, 3, 3, io, d);
}

/* Rule 4 of IP 3 on the device at n positions given after the geometry step (z0, lat0, x0 = geo2cart(0, lon0, lat0)), on
 * the points [a0, a0 + len) of the model's atmosphere: out [2 + ng + nw][n] -- p, T, q, k. */
int jur_kat_cloud_mean(jur_model_t *m, long n, int a0, int len, double const *z0, double const *lat0, double const (*x0)[3], double *out) {
  if (!m || n < 1 || !z0 || !lat0 || !x0 || !out) { jur_set_error("kat_cloud_mean: bad arguments"); return JUR_EINVAL; }
  if (m->ctl->ip != 3) { jur_set_error("kat_cloud_mean: the model was not created with ip = 3"); return JUR_EINVAL; }
  if (m->view.atm_np < 2 || m->cloud.np != m->view.atm_np) { jur_set_error("kat_cloud_mean: no atmosphere set"); return JUR_EINVAL; }
  if (a0 < 0 || len < 1 || (long)a0 + len > m->view.atm_np) { jur_set_error("kat_cloud_mean: points [%d, %d + %d) outside the atmosphere's %d", a0, a0, len, m->view.atm_np); return JUR_EINVAL; }
  int const nrow = 2 + m->view.ng + m->view.nw;
  HIPCHK(hipSetDevice(m->device));
  int rc = wait_done(m, m->stream);
  if (rc) return rc;
  double *d = NULL;
  size_t const N = (size_t)n;
  HIPCHK(hipMalloc((void **)&d, sizeof(double) * N * (size_t)(5 + nrow)));
  hipError_t e = hipMemcpy(d, z0, sizeof(double) * N, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + N, lat0, sizeof(double) * N, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + 2 * N, x0, sizeof(double) * 3 * N, hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(d); jur_set_error("kat_cloud_mean: upload failed"); return JUR_EHIP; }
  int const ek = jurk_kat_cloud_mean(&m->view, &m->cloud, n, a0, len, d, d + N, d + 2 * N, d + 5 * N, m->stream);
  if (ek) { jur_set_error("known-answer kernel not launched: %s", hipGetErrorString((hipError_t)ek)); rc = JUR_EHIP; }
  if (!rc && hipStreamSynchronize(m->stream) != hipSuccess) { jur_set_error("known-answer kernel failed"); rc = JUR_EHIP; }
  if (!rc && hipMemcpy(out, d + 5 * N, sizeof(double) * N * (size_t)nrow, hipMemcpyDeviceToHost) != hipSuccess) rc = JUR_EHIP;
  (void)hipFree(d);
  return rc;
}

int jur_cloud_lds_points(void) { return jurk_cloud_lds_points(); }

/* The ray tracer's LOS records point by point: the chunk loop of jur_curtis_godson_host (the same launches of
 * jurk_launch_trace, so jur_tune_trace selects the kernel as in production), each chunk gathered from the workspace
 * before the next one overwrites it.  An overflowing ray comes back clamped, with JUR_ENLOS. */
int jur_kat_traceray(jur_model_t *m, long nr, double const *const geom[7], double *los, double *tsurf, double *const tp[3],
                     int *np_out) {
  if (!m || nr < 1 || !geom || !los || !tsurf) { jur_set_error("kat_traceray: bad arguments"); return JUR_EINVAL; }
  if (m->view.atm_np < 2) { jur_set_error("kat_traceray: no atmosphere set"); return JUR_EINVAL; }
  view_set_k_zero(m);
  HIPCHK(hipSetDevice(m->device));
  int rc = ensure_workspace(m, nr);
  if (rc) return rc;
  long const Rt = m->use_trace_rays;
  hipStream_t s = m->stream;
  if ((rc = wait_done(m, s))) return rc;
  size_t const per_ray = (size_t)m->nfield * JUR_NLOS;
  double *d_geom = NULL, *d_los = NULL, *d_tsurf = NULL, *d_tp = NULL;
  int *d_np = NULL;
  hipError_t e = hipMalloc((void **)&d_geom, sizeof(double) * 7 * (size_t)nr);
  if (e == hipSuccess) e = hipMalloc((void **)&d_tp, sizeof(double) * 3 * (size_t)nr);
  if (e == hipSuccess) e = hipMalloc((void **)&d_np, sizeof(int) * (size_t)nr);
  if (e == hipSuccess) e = hipMalloc((void **)&d_tsurf, sizeof(double) * (size_t)nr);
  if (e == hipSuccess) e = hipMalloc((void **)&d_los, sizeof(double) * per_ray * (size_t)nr);
  if (e != hipSuccess) { rc = JUR_EHIP; jur_set_error("kat_traceray: hipMalloc failed"); goto done; }
  for (int k = 0; k < 7; k++)
    if (hipMemcpyAsync(d_geom + (size_t)k * nr, geom[k], sizeof(double) * nr, hipMemcpyHostToDevice, s) != hipSuccess) { rc = JUR_EHIP; goto done; }
  if (hipMemsetAsync(m->d_status, 0, sizeof(int), s) != hipSuccess) { rc = JUR_EHIP; goto done; }
  {
    for (long t0 = 0; t0 < nr; t0 += Rt) {
      jur_chunk_t c;
      memset(&c, 0, sizeof c);
      c.n = (int)((nr - t0 < Rt) ? nr - t0 : Rt);
      c.stride = (int)Rt;
      c.stride_eps = (int)m->use_rays;
      c.first = t0;
      c.order = NULL;
      for (int k = 0; k < 7; k++) c.geom[k] = d_geom + (size_t)k * nr;
      for (int k = 0; k < 3; k++) c.tp[k] = d_tp + (size_t)k * nr;
      c.np_out = d_np;
      c.np = m->d_np;
      c.tsurf = m->d_tsurf;
      c.los = m->d_los;
      c.eps = m->d_eps;
      c.status = m->d_status;
      int ek = jurk_launch_trace(&m->view, &m->track, &m->cloud, &c, s);
      if (!ek) ek = jurk_kat_los(&m->view, &c, d_los, d_tsurf, s);
      if (ek) { jur_set_error("kat_traceray: kernel launch failed: %s", hipGetErrorString((hipError_t)ek)); rc = JUR_EHIP; goto done; }
    }
    int status = 0;
    hipError_t ec = hipMemcpyAsync(los, d_los, sizeof(double) * per_ray * (size_t)nr, hipMemcpyDeviceToHost, s);
    if (ec == hipSuccess) ec = hipMemcpyAsync(tsurf, d_tsurf, sizeof(double) * nr, hipMemcpyDeviceToHost, s);
    for (int k = 0; k < 3 && tp && ec == hipSuccess; k++)
      ec = hipMemcpyAsync(tp[k], d_tp + (size_t)k * nr, sizeof(double) * nr, hipMemcpyDeviceToHost, s);
    if (np_out && ec == hipSuccess) ec = hipMemcpyAsync(np_out, d_np, sizeof(int) * nr, hipMemcpyDeviceToHost, s);
    if (ec == hipSuccess) ec = hipMemcpyAsync(&status, m->d_status, sizeof(int), hipMemcpyDeviceToHost, s);
    if (ec == hipSuccess) ec = hipStreamSynchronize(s);
    if (ec != hipSuccess) { jur_set_error("kat_traceray: copy back failed: %s", hipGetErrorString(ec)); rc = JUR_EHIP; goto done; }
    if (status & 1) { jur_set_error("Too many LOS points! (a ray needs %d or more)", JUR_NLOS); rc = JUR_ENLOS; }
  }
done:
  if (d_geom) (void)hipFree(d_geom);
  if (d_tp) (void)hipFree(d_tp);
  if (d_np) (void)hipFree(d_np);
  if (d_tsurf) (void)hipFree(d_tsurf);
  if (d_los) (void)hipFree(d_los);
  return rc;
}

/* ---- retrieval Jacobian -------------------------------------------------------- */
size_t jur_state_size(jur_model_t const *m, atm_t const *atm) { return jur_state_vector(m->ctl, atm, NULL, NULL, NULL); }

size_t jur_measurement_size(jur_model_t const *m, obs_t const *obs) {
  size_t n = 0;
  for (int ir = 0; ir < obs->nr; ir++)
    for (int id = 0; id < m->view.nd; id++) n += isfinite(obs->rad[ir][id]) ? 1 : 0;
  return n;
}

/* Forward-difference Jacobian (kernel(), jurassic.c:812-857) as ONE batched forward-model call:
 * the n perturbed atmospheres are stacked behind the unperturbed one as further profile slices
 * (time stamps shifted by j * span) and every ray is replicated once per slice. */
static int kernel_ld(jur_model_t *m, atm_t const *atm, obs_t *obs, double *k, size_t mrows, size_t ncols, size_t ldk);

int jur_kernel(jur_model_t *m, atm_t const *atm, obs_t *obs, double *k, size_t mrows, size_t ncols) {
  return kernel_ld(m, atm, obs, k, mrows, ncols, ncols);
}

static int kernel_ld(jur_model_t *m, atm_t const *atm, obs_t *obs, double *k, size_t mrows, size_t ncols, size_t ldk) {
  if (!m || !atm || !obs || !k) { jur_set_error("jur_kernel: null argument"); return JUR_EINVAL; }
  ctl_t const *ctl = m->ctl;
  int const np0 = atm->np, nr = obs->nr, nd = ctl->nd, ng = m->view.ng, nw = m->view.nw;
  if (np0 < 2 || np0 > JUR_NP || nr < 1 || nr > JUR_NR) { jur_set_error("jur_kernel: bad atm->np / obs->nr"); return JUR_EINVAL; }
  size_t const n = jur_state_vector(ctl, atm, NULL, NULL, NULL);
  if (n != ncols) { jur_set_error("jur_kernel: state vector has %zu elements, matrix has %zu columns", n, ncols); return JUR_EINVAL; }
  if (jur_measurement_size(m, obs) != mrows) { jur_set_error("jur_kernel: measurement vector size does not match the matrix rows"); return JUR_EINVAL; }
  double *x0 = (double *)malloc(sizeof(double) * (n + 1)), *hstep = (double *)malloc(sizeof(double) * (n + 1));
  int *iqa = (int *)malloc(sizeof(int) * (n + 1)), *ipa = (int *)malloc(sizeof(int) * (n + 1));
  jur_state_vector(ctl, atm, x0, iqa, ipa);

  size_t const ncopy = n + 1, nrow = 6 + (size_t)ng + nw;
  size_t const NT = ncopy * (size_t)np0, NRT = ncopy * (size_t)nr;
  double *h = (double *)malloc(sizeof(double) * nrow * NT);
  double *g = NULL;                                /* the model's pinned image of the call's arrays (ensure_io) */
  int rc = JUR_OK, stacked = 0;
  if (!x0 || !hstep || !iqa || !ipa || !h) { rc = JUR_ENOMEM; goto done; }
  if (hipSetDevice(m->device) != hipSuccess) { jur_set_error("jur_kernel: cannot select the device"); rc = JUR_EHIP; goto done; }
  if ((rc = ensure_io(m, (long)NRT, 1))) goto done;
  g = m->h_io;
  {
    double tmin = atm->time[0], tmax = atm->time[0];
    for (int i = 0; i < np0; i++) { tmin = fmin(tmin, atm->time[i]); tmax = fmax(tmax, atm->time[i]); }
    for (int i = 0; i < nr; i++) { tmin = fmin(tmin, obs->time[i]); tmax = fmax(tmax, obs->time[i]); }
    double const span = (tmax - tmin) + 1.0;
    for (size_t j = 0; j < ncopy; j++) {
      size_t const at = j * (size_t)np0;
      pack_atm_rows(m, atm, h, NT, at);
      if (j > 0) {  /* perturbation sizes, jurassic.c:831-837 */
        size_t const e = j - 1;
        int const iq = iqa[e];
        double hh;
        if (iq == 0) hh = fmax(fabs(0.01 * x0[e]), 1e-7);
        else if (iq == 1) hh = 1;
        else if (iq < 2 + ng) hh = fmax(fabs(0.01 * x0[e]), 1e-15);
        else hh = 1e-4;
        hstep[e] = hh;
        size_t const row = (iq == 0) ? 4 : (iq == 1) ? 5 : (size_t)(4 + iq);   /* q rows start at 6, k rows follow */
        h[row * NT + at + ipa[e]] = x0[e] + hh;
      }
      hydrostatic_rows(m, h, NT, at, np0);
      stack_times(h + at, atm->time, np0, (double)j * span);
    }
    m->h_atm_n = 0;                            /* the device no longer holds the caller's atmosphere */
    stacked = 1;
    rc = upload_atm_rows(m, h, (long)NT, JUR_ATM_PERTURBED);
    if (rc) goto done;
    double *geom[7], *tp[3], *rad, *tau;
    for (int q = 0; q < 7; q++) geom[q] = g + (size_t)q * NRT;
    rad = g + 7 * NRT;                             /* the image's layout: geom[7][N] | rad[N][nd] | tau[N][nd] | tp[3][N] */
    tau = rad + (size_t)nd * NRT;
    for (int q = 0; q < 3; q++) tp[q] = tau + (size_t)nd * NRT + (size_t)q * NRT;
    double const *src[7] = {obs->time, obs->obsz, obs->obslon, obs->obslat, obs->vpz, obs->vplon, obs->vplat};
    for (size_t j = 0; j < ncopy; j++)
      for (int i = 0; i < nr; i++) {
        size_t const r = j * (size_t)nr + i;
        geom[0][r] = stacked_ray_time(atm->time, np0, src[0][i], h + j * (size_t)np0, tmax + (ncopy + 1.0) * span);
        for (int q = 1; q < 7; q++) geom[q][r] = src[q][i];
        for (int id = 0; id < nd; id++) rad[r * nd + id] = obs->rad[i][id];   /* carries the NaN mask */
      }
    /* One batched call on device arrays; the difference quotients are formed there too (jur_kquot_kernel) and only
     * the unperturbed block and the quotients come back. */
    size_t const nq = (size_t)nr * nd, nrd = NRT * (size_t)nd;
    if ((long)(nq * n + n) > m->kq_cap) {
      if (m->d_kq) (void)hipFree(m->d_kq);
      if (m->h_kq) (void)hipHostFree(m->h_kq);
      m->d_kq = NULL; m->h_kq = NULL; m->kq_cap = 0;
      if (hipMalloc((void **)&m->d_kq, sizeof(double) * (nq * n + n)) != hipSuccess ||
          hipHostMalloc((void **)&m->h_kq, sizeof(double) * (nq * n + n), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError(); jur_set_error("jur_kernel: no memory for the quotients"); rc = JUR_ENOMEM; goto done;
      }
      m->kq_cap = (long)(nq * n + n);
    }
    hipStream_t const s = m->stream;
    double *const d_geom = m->d_io, *const d_rad = d_geom + 7 * NRT, *const d_tau = d_rad + nrd, *const d_tp = d_tau + nrd;
    double *const d_h = m->d_kq, *const d_kq = m->d_kq + n;
    int status = 0;
    memcpy(m->h_kq, hstep, sizeof(double) * n);
    hipError_t e = hipMemcpyAsync(d_geom, g, sizeof(double) * (7 * NRT + nrd), hipMemcpyHostToDevice, s);   /* geometry | input radiances */
    if (e == hipSuccess) e = hipMemcpyAsync(d_h, m->h_kq, sizeof(double) * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(m->d_status, 0, sizeof(int), s);
    if (e != hipSuccess) { jur_set_error("jur_kernel: %s", hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
    if ((rc = jur_formod_device(m, (long)NRT, d_geom, d_rad, d_tau, d_tp, NULL, m->d_status, s))) goto done;
    if (jurk_launch_kquot((long)nq, (long)n, d_rad, d_h, d_kq, s)) { jur_set_error("jur_kernel: quotient kernel launch failed"); rc = JUR_EHIP; goto done; }
    double *const kq = m->h_kq + n;
    e = hipMemcpyAsync(kq, d_kq, sizeof(double) * nq * n, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(rad, d_rad, sizeof(double) * nq, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(tau, d_tau, sizeof(double) * nq, hipMemcpyDeviceToHost, s);
    for (int q = 0; q < 3 && e == hipSuccess; q++) e = hipMemcpyAsync(tp[q], d_tp + (size_t)q * NRT, sizeof(double) * nr, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&status, m->d_status, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { jur_set_error("jur_kernel: %s", hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
    if (status) { jur_set_error("Too many LOS points!"); rc = JUR_ENLOS; goto done; }
    for (int i = 0; i < nr; i++) {   /* unperturbed result back to the caller, as kernel() leaves it */
      for (int id = 0; id < nd; id++) { obs->rad[i][id] = rad[(size_t)i * nd + id]; obs->tau[i][id] = tau[(size_t)i * nd + id]; }
      for (int id = nd; id < JUR_ND; id++) { obs->rad[i][id] = 0.0; obs->tau[i][id] = 1.0; }
      obs->tpz[i] = tp[0][i]; obs->tplon[i] = tp[1][i]; obs->tplat[i] = tp[2][i];
    }
    size_t row = 0;
    for (size_t q = 0; q < nq; q++) {              /* rows of the finite measurements (obs2y, jurassic.c:1527-1541) */
      if (!isfinite(rad[q])) continue;
      if (row < mrows) memcpy(k + row * ldk, kq + q * n, sizeof(double) * n);
      row++;
    }
    if (row != mrows) { jur_set_error("jur_kernel: %zu finite measurements after the forward model, the matrix has %zu rows", row, mrows); rc = JUR_EINVAL; }
  }
done:
  free(x0); free(hstep); free(iqa); free(ipa); free(h);
  /* leave the model with the caller's atmosphere -- after an error too (JUR_ENLOS, a failed launch): never with the
   * stacked one, which later calls would accept; if it cannot go back, with none ("no atmosphere set") */
  if (rc == JUR_OK) rc = jur_model_set_atm(m, atm);
  else if (stacked) {
    char msg[512];
    snprintf(msg, sizeof msg, "%s", jur_last_error());
    if (jur_model_set_atm(m, atm) != JUR_OK) { m->view.atm_np = 0; m->h_atm_n = 0; }
    jur_set_error("%s", msg);
  }
  return rc;
}

/* ---- block Jacobian of a scene -------------------------------------------------- */

/* Sibling of upload_atm_rows for rows that a kernel is about to write on the device: makes room for nt points in the
 * model's slab, waits for readers of the old rows and points the view at the new ones.  No host image of these rows
 * exists, so the facts come from the base atmosphere they are stacked from: atm_sorted, atm_maxslice and the altitude
 * range are the base's (every copy is a slice of it under one time stamp of its own), the slices the base's plus one
 * per copy.  The caller fills the rows on the model's stream and then runs jurk_prepare_atm on them. */
static int install_stacked_rows(jur_model_t *m, atm_t const *base, long nt, long ncopies) {
  HIPCHK(hipSetDevice(m->device));
  jur_view_t *v = &m->view;
  size_t const ng = (size_t)v->ng, nrow = 6 + ng + (size_t)v->nw, n = (size_t)nt;
  v->atm_np = 0;
  m->atm_k_zero = 0; v->atm_k_zero = 0;   /* JUR_ATM_DEVICE: no host image of these rows, and they may raise an extinction */
  if (nt > m->atm_cap) {
    if (m->d_atm) (void)hipFree(m->d_atm);
    m->d_atm = NULL;
    m->atm_cap = 0;
    HIPCHK(hipMalloc(&m->d_atm, sizeof(double) * (nrow + 1) * n));
    m->atm_cap = (int)nt;
  }
  if (m->have_done) {
    HIPCHK(hipEventSynchronize(m->ev_done));
    m->have_done = 0;
  }
  derive_atm_facts(m, base->time, base->z, base->np);
  m->atm_slices += (int)ncopies;
  double const *d = (double const *)m->d_atm;
  v->atm_np = (int)nt;
  v->atm_time = d; v->atm_z = d + n; v->atm_lon = d + 2 * n; v->atm_lat = d + 3 * n;
  v->atm_p = d + 4 * n; v->atm_t = d + 5 * n;
  v->atm_q = d + 6 * n; v->atm_k = d + (6 + ng) * n;
  v->atm_pslope = d + nrow * n;
  return JUR_OK;
}

/* what jur_normal_scene_host adds to a call: measurements and weights in, the sums per slice out */
typedef struct {
  double const *y, *weight;
  double *A, *b, *cost;
  long *nlive;
} scene_normal_t;

/* ---- Levenberg-Marquardt step of the slices (jur_solve_slices_host, jur_step_scene_host) ------------------------- */
/* what jur_step_scene_host adds to jur_normal_scene_host */
typedef struct { jur_solve_in_t const *in; jur_solve_out_t const *out; } scene_solve_t;

/* the refusals that need no sizes */
static int solve_check_args(char const *who, jur_solve_in_t const *in, jur_solve_out_t const *out) {
  if (!in || !out) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  if (in->nlam < 1) { jur_set_error("%s: nlam = %d: at least one damping is needed", who, in->nlam); return JUR_EINVAL; }
  if (in->mode != JUR_DAMP_MARQUARDT && in->mode != JUR_DAMP_PRIOR) { jur_set_error("%s: unknown mode %d", who, in->mode); return JUR_EINVAL; }
  if (!in->prior_ivar != !in->prior_dx) {
    jur_set_error("%s: %s without %s: the prior is given as a pair", who, in->prior_ivar ? "prior_ivar" : "prior_dx",
                  in->prior_ivar ? "prior_dx" : "prior_ivar");
    return JUR_EINVAL;
  }
  if (in->mode == JUR_DAMP_PRIOR && !in->prior_ivar) { jur_set_error("%s: JUR_DAMP_PRIOR without a prior", who); return JUR_EINVAL; }
  if (!in->lam || !out->dx || !out->pred || !out->status) {
    jur_set_error("%s: null argument (%s)", who, !in->lam ? "lam" : !out->dx ? "dx" : !out->pred ? "pred" : "status");
    return JUR_EINVAL;
  }
  return JUR_OK;
}

/* the dampings and the prior of nslice systems laid out by wptr */
static int solve_check_values(char const *who, long nslice, long const *wptr, jur_solve_in_t const *in) {
  for (int l = 0; l < in->nlam; l++)
    for (long q = 0; q < nslice; q++) {
      double const v = in->lam[(size_t)l * (size_t)nslice + (size_t)q];
      if (!(v >= 0) || isinf(v)) {
        jur_set_error("%s: lam of slice %ld, damping %d is %g: negative or not finite", who, q, l, v);
        return JUR_EINVAL;
      }
    }
  if (in->prior_ivar)
    for (long q = 0; q < nslice; q++)
      for (long e = wptr[q]; e < wptr[q + 1]; e++) {
        double const r = in->prior_ivar[e], d = in->prior_dx[e];
        if (!(r >= 0) || isinf(r)) {
          jur_set_error("%s: prior_ivar of slice %ld, element %ld is %g: negative or not finite", who, q, e - wptr[q], r);
          return JUR_EINVAL;
        }
        if (!isfinite(d)) {
          jur_set_error("%s: prior_dx of slice %ld, element %ld is %g: not finite", who, q, e - wptr[q], d);
          return JUR_EINVAL;
        }
      }
  return JUR_OK;
}

/* The solver's part of the slab beside A and b, as offsets in doubles from its start: M, the scratch copy of the
 * matrices; live, the liveness of one damping; for all dampings dx | pred | lam; the prior pair r | d (empty without a
 * prior); stat (ints, rounded up to doubles); with a full prior precision behind those Ap, the assembled matrices A + P
 * (+ lam P), g and zl, the zero dampings.  end: the doubles of the part.  Whoever sizes or reads the part asks here. */
typedef struct { size_t M, live, dx, pred, lam, r, d, stat, Ap, g, zl, end; } solve_layout_t;

static solve_layout_t solve_layout(size_t na, size_t nb, size_t ns, size_t nlam, int prior, int full) {
  size_t const npr = prior ? nb : 0;
  solve_layout_t o;
  o.M = 0; o.live = o.M + na; o.dx = o.live + nb; o.pred = o.dx + nlam * nb; o.lam = o.pred + nlam * ns; o.r = o.lam + nlam * ns;
  o.d = o.r + npr; o.stat = o.d + npr; o.Ap = o.stat + (nlam * ns + 1) / 2; o.g = o.Ap + (full ? na : 0); o.zl = o.g + (full ? nb : 0);
  o.end = o.zl + (full ? ns : 0);
  return o;
}

/* Enqueues on s: the uploads of the dampings and the prior, one launch per damping over the one scratch (stream order
 * protects the copy-out of L), the copies home.  The caller waits for the stream before the host arrays go. */
static int solve_enqueue(jur_model_t *m, hipStream_t s, char const *who, long nslice, long na, long nb, long const *d_wptr,
                         long const *d_aptr, double const *d_A, double const *d_b, double *W, jur_solve_in_t const *in,
                         jur_solve_out_t const *out, int const *d_state, double const *d_R) {
  /* d_state (jur_retrieve_scene_host): the prior pair is on the device already, the steps stay there, and a system
   * whose state is not 0 is left alone.  d_R (a full prior precision is set): the solve kernel runs on A + P and g as
   * jurk_scene_prior_assemble forms them, without a prior of its own; under JUR_DAMP_PRIOR on A + P + lam P with lam = 0,
   * and jurk_scene_prior_pred then writes pred */
  int const resident = d_state != NULL;
  size_t const NA = (size_t)na, NB = (size_t)nb, NS = (size_t)nslice, NL = (size_t)in->nlam, npr = in->prior_ivar ? NB : 0;
  solve_layout_t const o = solve_layout(NA, NB, NS, NL, npr != 0, d_R != NULL);
  double *const dM = W + o.M, *const dlive = W + o.live, *const ddx = W + o.dx, *const dpred = W + o.pred, *const dlam = W + o.lam,
         *const dr = W + o.r, *const dd = W + o.d;
  int *const dstat = (int *)(W + o.stat);
  hipError_t e = hipMemcpyAsync(dlam, in->lam, sizeof(double) * NL * NS, hipMemcpyHostToDevice, s);
  if (npr && !resident && e == hipSuccess) e = hipMemcpyAsync(dr, in->prior_ivar, sizeof(double) * NB, hipMemcpyHostToDevice, s);
  if (npr && !resident && e == hipSuccess) e = hipMemcpyAsync(dd, in->prior_dx, sizeof(double) * NB, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); return JUR_EHIP; }
  jur_scene_solve_t q;
  memset(&q, 0, sizeof q);
  q.nslice = nslice; q.wptr = d_wptr; q.aptr = d_aptr; q.A = d_A; q.b = d_b;
  q.prior_ivar = npr ? dr : NULL; q.prior_dx = npr ? dd : NULL; q.mode = in->mode;
  q.M = dM; q.live = dlive; q.state = d_state;
  jur_scene_pasm_t pa;
  jur_scene_pquad_t pq;
  memset(&pa, 0, sizeof pa); memset(&pq, 0, sizeof pq);
  int const by_prior = in->mode == JUR_DAMP_PRIOR;
  if (d_R) {
    double *const dAp = W + o.Ap, *const dg = W + o.g, *const dzl = W + o.zl;
    pa.nslice = nslice; pa.wptr = d_wptr; pa.aptr = d_aptr; pa.A = d_A; pa.b = d_b; pa.R = d_R; pa.ivar = dr; pa.d = dd;
    pa.M = dAp; pa.g = dg; pa.state = d_state;
    pq.nslice = nslice; pq.nvec = 1; pq.wptr = d_wptr; pq.aptr = d_aptr; pq.R = d_R; pq.state = d_state;
    pq.ivar = dr; pq.g = dg; pq.live = dlive;
    q.A = dAp; q.b = dg; q.prior_ivar = NULL; q.prior_dx = NULL; q.mode = JUR_DAMP_MARQUARDT;
    if (by_prior && hipMemsetAsync(dzl, 0, sizeof(double) * NS, s) != hipSuccess) { (void)hipGetLastError(); jur_set_error("%s: memset failed", who); return JUR_EHIP; }
    /* without JUR_DAMP_PRIOR one assembly serves every damping: fma(lam, D, D) is the solve kernel's */
    if (!by_prior && SCENE_TIMED(m, s, jurk_scene_prior_assemble(&pa, nb, s))) return launch_failed("%s: prior assembly kernel launch failed", who);
  }
  for (size_t l = 0; l < NL; l++) {
    q.lam = dlam + l * NS; q.dx = ddx + l * NB; q.pred = dpred + l * NS; q.status = dstat + l * NS;
    int const ti = scene_timed_begin(m, s);
    int ek = 0;
    if (d_R && by_prior) {
      pa.lam = dlam + l * NS;
      if (l > 0) { pa.b = NULL; pa.d = NULL; }      /* (g does not depend on the damping) */
      ek = jurk_scene_prior_assemble(&pa, nb, s);
      q.lam = W + o.zl;                             /* (the zero dampings) */
    }
    if (!ek) ek = jurk_scene_solve(&q, s);
    if (!ek && d_R && by_prior) {
      pq.v = q.dx; pq.out = q.pred; pq.lam = dlam + l * NS; pq.status = q.status;
      ek = jurk_scene_prior_pred(&pq, s);
    }
    scene_timed_end(m, ti, s);
    if (ek) { jur_set_error("%s: solve kernel launch failed", who); return JUR_EHIP; }
    if (out->L && NA) e = hipMemcpyAsync(out->L + l * NA, dM, sizeof(double) * NA, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); return JUR_EHIP; }
  }
  if (NB && !resident) e = hipMemcpyAsync(out->dx, ddx, sizeof(double) * NL * NB, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(out->pred, dpred, sizeof(double) * NL * NS, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(out->status, dstat, sizeof(int) * NL * NS, hipMemcpyDeviceToHost, s);
  if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); return JUR_EHIP; }
  return JUR_OK;
}

/* ---- posterior diagnostics of the slices (jur_diagnose_slices_host, jur_diagnose_scene_host) ------------------------ */
/* what jur_diagnose_scene_host adds to jur_normal_scene_host */
/* ... and what jur_gain_scene_host adds to that (gin == NULL: the diagnostics alone) */
typedef struct { double const *prior_ivar; jur_diag_out_t const *out; jur_gain_in_t const *gin; jur_gain_out_t const *gout; } scene_diag_t;

/* The diagnostics' part of the slab beside A, as offsets in doubles from its start: L | S | K (the AVK), then live | z |
 * zero (the solve's b and prior_dx) | r (prior_ivar, empty without a prior), vec (the four vectors), lam (zeros) | pred |
 * dofs, stat (the ints status [ns] | imap [2 ninv] | tmap [3 ntile], rounded up to doubles); with a full prior precision
 * behind those P (A + P, then P alone, for the smoothing error) and SP (S P).  end: the doubles of the part. */
typedef struct { size_t L, S, K, live, z, zero, r, vec, lam, pred, dofs, stat, P, SP, end; } diag_layout_t;

static diag_layout_t diag_layout(size_t na, size_t nb, size_t ns, int prior, int full, size_t ninv, size_t ntile) {
  diag_layout_t o;
  o.L = 0; o.S = o.L + na; o.K = o.S + na; o.live = o.K + na; o.z = o.live + nb; o.zero = o.z + nb; o.r = o.zero + nb;
  o.vec = o.r + (prior ? nb : 0); o.lam = o.vec + 4 * nb; o.pred = o.lam + ns; o.dofs = o.pred + ns; o.stat = o.dofs + ns;
  o.P = o.stat + (ns + 2 * ninv + 3 * ntile + 1) / 2; o.SP = o.P + (full ? na : 0); o.end = o.SP + (full ? na : 0);
  return o;
}

/* Enqueues on s: the uploads of the prior and the block maps (hmap: imap | tmap), the factorisation by the solve kernel
 * (lam = 0, zero right-hand side, zero prior_dx), the inverse, the product and the vectors, the copies home.  The caller
 * waits for the stream before the host arrays go. */
static int diag_enqueue(jur_model_t *m, hipStream_t s, char const *who, long nslice, long na, long nb, long const *d_wptr,
                        long const *d_aptr, double const *d_A, double *W, double const *prior_ivar, jur_diag_out_t const *out,
                        long ninv, long ntile, int const *hmap, double const *d_R) {
  /* d_R (a full prior precision is set): the factor is that of A + P as jurk_scene_prior_assemble forms it, and
   * sigma_smooth comes from the product S P */
  size_t const NA = (size_t)na, NB = (size_t)nb, NS = (size_t)nslice, npr = prior_ivar ? NB : 0;
  diag_layout_t const o = diag_layout(NA, NB, NS, npr != 0, d_R != NULL, (size_t)ninv, (size_t)ntile);
  double *const dL = W + o.L, *const dS = W + o.S, *const dK = W + o.K, *const dlive = W + o.live, *const dz = W + o.z, *const dzero = W + o.zero,
         *const dr = W + o.r, *const dvec = W + o.vec, *const dlam = W + o.lam, *const dpred = W + o.pred, *const ddofs = W + o.dofs;
  int *const dstat = (int *)(W + o.stat), *const dimap = dstat + NS, *const dtmap = dimap + 2 * (size_t)ninv;
  hipError_t e = hipMemsetAsync(dlam, 0, sizeof(double) * NS, s);
  if (NB && e == hipSuccess) e = hipMemsetAsync(dzero, 0, sizeof(double) * NB, s);
  if (npr && e == hipSuccess) e = hipMemcpyAsync(dr, prior_ivar, sizeof(double) * NB, hipMemcpyHostToDevice, s);
  if (ninv + ntile > 0 && e == hipSuccess)
    e = hipMemcpyAsync(dimap, hmap, sizeof(int) * (2 * (size_t)ninv + 3 * (size_t)ntile), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); return JUR_EHIP; }
  jur_scene_solve_t q;
  memset(&q, 0, sizeof q);
  q.nslice = nslice; q.wptr = d_wptr; q.aptr = d_aptr; q.A = d_A; q.b = dzero;
  q.prior_ivar = npr ? dr : NULL; q.prior_dx = npr ? dzero : NULL; q.mode = JUR_DAMP_MARQUARDT;
  q.M = dL; q.live = dlive; q.lam = dlam; q.dx = dz; q.pred = dpred; q.status = dstat;
  jur_scene_diag_t d;
  memset(&d, 0, sizeof d);
  d.nslice = nslice; d.wptr = d_wptr; d.aptr = d_aptr; d.A = d_A; d.prior_ivar = npr ? dr : NULL;
  d.L = dL; d.live = dlive; d.status = dstat; d.imap = dimap; d.tmap = dtmap; d.S = dS; d.avk = dK;
  d.sigma = dvec; d.sigma_noise = dvec + NB; d.sigma_smooth = dvec + 2 * NB; d.avk_diag = dvec + 3 * NB; d.dofs = ddofs;
  int const ti = scene_timed_begin(m, s);
  int ek = 0;
  jur_scene_pasm_t pa;
  memset(&pa, 0, sizeof pa);
  if (d_R) {
    pa.nslice = nslice; pa.wptr = d_wptr; pa.aptr = d_aptr; pa.A = d_A; pa.R = d_R; pa.ivar = dr;
    pa.M = W + o.P;
    ek = jurk_scene_prior_assemble(&pa, nb, s);
    q.A = pa.M; q.prior_ivar = NULL; q.prior_dx = NULL;
    d.prior_ivar = NULL;                          /* (the rows kernel writes sqrt(0); jurk_scene_prior_smooth the value) */
  }
  if (!ek) ek = jurk_scene_solve(&q, s);
  if (!ek) ek = jurk_scene_diag(&d, ninv, ntile, nb, s);
  if (!ek && d_R) {
    pa.A = NULL;                                  /* P alone where A + P lay: the factor has been taken */
    ek = jurk_scene_prior_assemble(&pa, nb, s);
    jur_scene_diag_t d2 = d;
    d2.A = W + o.P; d2.avk = W + o.SP;
    if (!ek) ek = jurk_scene_prior_smooth(&d2, ntile, nb, s);
  }
  scene_timed_end(m, ti, s);
  if (ek) { jur_set_error("%s: diagnostics kernel launch failed", who); return JUR_EHIP; }
  if (NB) {
    e = hipMemcpyAsync(out->sigma, d.sigma, sizeof(double) * NB, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(out->sigma_noise, d.sigma_noise, sizeof(double) * NB, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(out->sigma_smooth, d.sigma_smooth, sizeof(double) * NB, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(out->avk_diag, d.avk_diag, sizeof(double) * NB, hipMemcpyDeviceToHost, s);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out->dofs, ddofs, sizeof(double) * NS, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(out->status, dstat, sizeof(int) * NS, hipMemcpyDeviceToHost, s);
  if (NA && out->S && e == hipSuccess) e = hipMemcpyAsync(out->S, dS, sizeof(double) * NA, hipMemcpyDeviceToHost, s);
  if (NA && out->avk && e == hipSuccess) e = hipMemcpyAsync(out->avk, dK, sizeof(double) * NA, hipMemcpyDeviceToHost, s);
  if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); return JUR_EHIP; }
  return JUR_OK;
}

/* the block maps of nslice systems in one malloc'ed array imap | tmap (NULL with JUR_OK where there is no block) */
static int diag_maps_make(char const *who, long nslice, long const *wptr, long *ninv, long *ntile, int **hmap) {
  *hmap = NULL;
  *ninv = jur_diag_maps(nslice, wptr, NULL, NULL, ntile);
  if (*ninv > 0x7fffffffL || *ntile > 0x7fffffffL || wptr[nslice] / 4 >= 0x7fffffffL) {
    jur_set_error("%s: 2^31 blocks: call with fewer systems at a time", who);
    return JUR_EINVAL;
  }
  if (*ninv == 0) return JUR_OK;
  *hmap = (int *)malloc(sizeof(int) * (2 * (size_t)*ninv + 3 * (size_t)*ntile));
  if (!*hmap) { jur_set_error("%s: out of memory", who); return JUR_ENOMEM; }
  (void)jur_diag_maps(nslice, wptr, *hmap, *hmap + 2 * *ninv, NULL);
  return JUR_OK;
}

/* ---- gain matrix and error budget of the slices (jur_gain_slices_host, jur_gain_scene_host) --------------------------- */
/* The gain's part of the slab, as offsets in doubles from its start: gain (nk doubles, laid out as the blocks: never the
 * blocks themselves, which the tiles of other elements still read) | sigc [ncomp][nb] | var [ncomp][nrd] | weff [nrd] |
 * map (the ints of the tile map [3 ntile], rounded up to doubles).  end: the doubles of the part. */
typedef struct { size_t gain, sigc, var, weff, map, end; } gain_layout_t;

static gain_layout_t gain_layout(size_t nk, size_t nb, size_t nrd, size_t ncomp, size_t ntile) {
  gain_layout_t o;
  o.gain = 0; o.sigc = o.gain + nk; o.var = o.sigc + ncomp * nb; o.weff = o.var + ncomp * nrd; o.map = o.weff + nrd;
  o.end = o.map + (3 * ntile + 1) / 2;
  return o;
}

/* the tile map of the gain kernel in one malloc'ed array (NULL with JUR_OK where there is no tile) */
static int gain_maps_make(char const *who, long nslice, long const *wptr, long const *sptr, int nd, long *ntile, int **hmap) {
  *hmap = NULL;
  *ntile = jur_gain_maps(nslice, wptr, sptr, nd, NULL);
  if (*ntile < 0 || *ntile > 0x7fffffffL) {
    jur_set_error("%s: 2^31 gain tiles or measurements of one slice: call with the rays of fewer slices at a time", who);
    return JUR_EINVAL;
  }
  if (*ntile == 0) return JUR_OK;
  *hmap = (int *)malloc(sizeof(int) * 3 * (size_t)*ntile);
  if (!*hmap) { jur_set_error("%s: out of memory", who); return JUR_ENOMEM; }
  (void)jur_gain_maps(nslice, wptr, sptr, nd, *hmap);
  return JUR_OK;
}

/* Enqueues on s: the uploads of the variances and the tile map, the gain and budget kernels, the copies home of what was
 * asked for.  q comes with everything but weff, var, gmap, gain and sigc, which lie in the part W of the slab (weff
 * filled by the caller); nk: the doubles of all blocks.  gain_at (jur_param_scene_host): the gain is written there and the
 * part has no room for it.  The caller waits for the stream before the host arrays go. */
static int gain_enqueue(jur_model_t *m, hipStream_t s, char const *who, jur_scene_gain_t *q, double *W, size_t nk, long ntile,
                        long ngroups, int const *hmap, jur_gain_in_t const *in, jur_gain_out_t const *out, double *gain_at) {
  size_t const NB = (size_t)q->nb, NRD = (size_t)q->nrd, NC = (size_t)in->ncomp;
  gain_layout_t const o = gain_layout(gain_at ? 0 : nk, NB, NRD, NC, (size_t)ntile);
  hipError_t e = hipSuccess;
  if (NC && NRD) e = hipMemcpyAsync(W + o.var, in->var, sizeof(double) * NC * NRD, hipMemcpyHostToDevice, s);
  if (ntile > 0 && e == hipSuccess) e = hipMemcpyAsync(W + o.map, hmap, sizeof(int) * 3 * (size_t)ntile, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); return JUR_EHIP; }
  q->ncomp = in->ncomp;
  q->weff = W + o.weff; q->var = W + o.var; q->gmap = (int const *)(W + o.map); q->gain = gain_at ? gain_at : W + o.gain; q->sigc = W + o.sigc;
  if (SCENE_TIMED(m, s, jurk_scene_gain(q, ntile, ngroups, s))) return launch_failed("%s: gain kernel launch failed", who);
  if (nk && out->gain) e = hipMemcpyAsync(out->gain, q->gain, sizeof(double) * nk, hipMemcpyDeviceToHost, s);
  if (NC && NB && e == hipSuccess) e = hipMemcpyAsync(out->sigma_comp, q->sigc, sizeof(double) * NC * NB, hipMemcpyDeviceToHost, s);
  if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); return JUR_EHIP; }
  return JUR_OK;
}

/* ---- trial states and the retrieval loop (jur_trial_scene_host, jur_retrieve_scene_host) ----------------------------- */
/* The row of the stacked atmosphere that holds state quantity iq (jur_state_vector's: 0 p, 1 T, then the gases, then the
 * windows): p and T are rows 4 and 5, the q rows start at 6, the k rows follow.  And back: the array of atm a row is. */
static int scene_row_of(int iq) { return (iq == 0) ? 4 : (iq == 1) ? 5 : 4 + iq; }
static double *scene_row_array(atm_t *atm, int ng, int row) {
  return row == 4 ? atm->p : row == 5 ? atm->t : row < 6 + ng ? atm->q[row - 6] : atm->k[row - 6 - ng];
}

/* Host image of what the trial kernels index by: two blocks, each uploaded with one copy.
 * longs: wptr[ns + 1] | off[ncopy + 1] | sptr[ns + 1];  ints: cdesc[3 ncopy] (first | prow = -1 | pip = 0 of every copy,
 * for jur_scene_stack_kernel) | sfirst[ns] | erow[nb] | eip[nb] | tcopy0[nr] | srays[nlist]
 * box: the box on the state per element, lo | hi (NULL: the model has none) */
typedef struct {
  int ntrial;
  long nslice, nb, ncopy, nt, nr, nlist;
  long *longs, *wptr, *off, *sptr;
  int *ints, *cdesc, *sfirst, *erow, *eip, *tcopy0, *srays;
  size_t nlong, nint;
  double *box;
} trial_plan_t;

static void trial_plan_free(trial_plan_t *p) { free(p->longs); free(p->ints); free(p->box); memset(p, 0, sizeof *p); }

static int trial_plan_make(trial_plan_t *p, char const *who, jur_model_t const *m, atm_t const *atm, int ntrial, long nr, long nslice,
                           jur_scene_slice_t const *sl, int const *sid) {
  ctl_t const *const ctl = m->ctl;
  memset(p, 0, sizeof *p);
  size_t const NS = (size_t)nslice, NR = (size_t)nr;
  long nb = 0, nt = atm->np;
  for (long q = 0; q < nslice; q++) { nb += sl[q].nel; nt += (long)ntrial * sl[q].len; }
  long const ncopy = 1 + nslice * ntrial;
  p->ntrial = ntrial; p->nslice = nslice; p->nb = nb; p->ncopy = ncopy; p->nt = nt; p->nr = nr;
  p->nlong = 2 * (NS + 1) + (size_t)ncopy + 1;
  p->nint = 3 * (size_t)ncopy + NS + 2 * (size_t)nb + 2 * NR;
  p->longs = (long *)calloc(p->nlong, sizeof(long));
  p->ints = (int *)calloc(p->nint ? p->nint : 1, sizeof(int));
  int *scratch = (int *)malloc(sizeof(int) * 2 * (size_t)(nb ? nb : 1));
  if (!p->longs || !p->ints || !scratch) { free(scratch); trial_plan_free(p); return JUR_ENOMEM; }
  p->wptr = p->longs; p->off = p->wptr + NS + 1; p->sptr = p->off + ncopy + 1;
  p->cdesc = p->ints; p->sfirst = p->cdesc + 3 * ncopy; p->erow = p->sfirst + NS; p->eip = p->erow + nb;
  p->tcopy0 = p->eip + nb; p->srays = p->tcopy0 + NR;
  int *const cfirst = p->cdesc, *const prow = p->cdesc + ncopy;
  cfirst[0] = 0; prow[0] = -1;
  p->off[0] = 0; p->off[1] = atm->np;
  int rc = JUR_OK;
  for (long q = 0; q < nslice && !rc; q++) {
    p->wptr[q + 1] = p->wptr[q] + sl[q].nel;
    p->sfirst[q] = sl[q].first;
    long const n = jur_scene_slice_elements(ctl, atm, sl[q].first, sl[q].len, NULL, scratch, scratch + nb);
    if (n != sl[q].nel) { jur_set_error("%s: layout out of step", who); rc = JUR_EINVAL; break; }
    for (long e = 0; e < n; e++) {
      p->erow[p->wptr[q] + e] = scene_row_of(scratch[e]);
      p->eip[p->wptr[q] + e] = scratch[nb + e];
    }
    for (int t = 0; t < ntrial; t++) {
      long const j = 1 + q * ntrial + t;
      cfirst[j] = sl[q].first; prow[j] = -1;
      p->off[j + 1] = p->off[j] + sl[q].len;
    }
  }
  free(scratch);
  if (rc) { trial_plan_free(p); return rc; }
  for (long r = 0; r < nr; r++) p->tcopy0[r] = sid[r] >= 0 ? (int)(1 + (long)sid[r] * ntrial) : 0;
  p->nlist = jur_scene_rays_by_slice(nr, nslice, sid, p->sptr, p->srays);
  if (m->sb_nq && nb > 0) {
    if (!(p->box = (double *)malloc(sizeof(double) * 2 * (size_t)nb))) { trial_plan_free(p); return JUR_ENOMEM; }
    jur_state_bounds_expand(m->sb_lo, m->sb_hi, nb, p->erow, p->box, p->box + nb);
  }
  return JUR_OK;
}

/* a field of view in a call: the kernel's arguments (shape, status word and the rays' time stamps and view-point altitudes
 * are the call's; the pass fills in the rest), the effective mask [rays][nd] on the device and, for the Jacobian passes,
 * the convolved transmittances by ray [rays][nd] */
typedef struct { jur_scene_fov_t k; double const *live; double *tau; } scene_fov_t;

/* The device views of a trial pass, which trial_run consumes.  tq.R (a full prior precision is set) and of.flag
 * (JUR_OVERFLOW_ISOLATE) say whether the last two take part. */
typedef struct { jur_scene_stack_t sk; jur_scene_trial_t st; jur_scene_trial_pass_t ps; jur_scene_pquad_t tq; jur_scene_ovfold_t of; } trial_dev_t;

/* ... of the plan pl, whose two blocks lie at Lp and Ip on the device, over the call's arrays there.  ivar, xa: the
 * diagonal prior or both NULL; box: lo | hi or NULL; d_R: the full prior precision or NULL, laid out by aptr, with v for
 * xa - (x + dx) of every trial; oflag, opart: the trials' overflow flags and the fold's counts, or NULL; state, choice: of
 * the slices of a retrieval, or NULL. */
static void trial_dev_fill(trial_dev_t *td, jur_model_t const *m, trial_plan_t const *pl, int np0, double tmax, double span,
                           long const *Lp, int const *Ip, double *base, double const *geom, double const *in_rad, int const *first,
                           int const *len, double const *y, double const *weight, double const *dx, double const *ivar,
                           double const *xa, double *prior, double *cost, double const *box, double const *d_R, long const *aptr,
                           double *v, int *oflag, long *opart, int *state, int const *choice) {
  long const *const d_off = Lp + (pl->off - pl->longs);
  memset(td, 0, sizeof *td);
  jur_scene_stack_t *const sk = &td->sk;
  sk->ncopy = (int)pl->ncopy; sk->np0 = np0; sk->nrow = 6 + m->view.ng + m->view.nw; sk->ng = m->view.ng; sk->nt = pl->nt;
  sk->off = d_off; sk->first = Ip; sk->prow = Ip + pl->ncopy; sk->pip = Ip + 2 * pl->ncopy;
  sk->base = base; sk->tmax = tmax; sk->span = span;
  jur_scene_trial_t *const st = &td->st;
  st->nslice = pl->nslice; st->ntrial = pl->ntrial; st->np0 = np0; st->nt = pl->nt;
  st->wptr = Lp; st->off = d_off; st->sfirst = Ip + (pl->sfirst - pl->ints); st->erow = Ip + (pl->erow - pl->ints);
  st->eip = Ip + (pl->eip - pl->ints); st->state = state; st->choice = choice;
  st->base = base; st->dx = dx; st->ivar = ivar; st->xa = xa; st->prior = prior;
  if (box) { st->lo = box; st->hi = box + pl->nb; }
  jur_scene_trial_pass_t *const ps = &td->ps;
  ps->nr = pl->nr; ps->nd = m->ctl->nd; ps->ntrial = pl->ntrial; ps->first = first; ps->len = len; ps->tcopy0 = Ip + (pl->tcopy0 - pl->ints);
  ps->off = d_off; ps->in_geom = geom; ps->in_rad = in_rad; ps->nslice = pl->nslice; ps->sptr = Lp + (pl->sptr - pl->longs);
  ps->srays = Ip + (pl->srays - pl->ints); ps->state = state; ps->y = y; ps->weight = weight; ps->cost = cost;
  td->tq.nslice = pl->nslice; td->tq.nvec = pl->ntrial; td->tq.wptr = Lp; td->tq.aptr = aptr; td->tq.R = d_R; td->tq.v = v;
  td->tq.out = prior; td->tq.state = state;
  if (oflag) { td->of.nslice = pl->nslice; td->of.ntrial = pl->ntrial; td->of.flag = oflag; td->of.state = state; td->of.cost = cost; td->of.part = opart; }
}

/* One trial pass over the device: stacks the trial copies from the base rows (st->base), moves the elements by st->dx,
 * forms the prior terms (or zeroes them), traces the rays of every pass and continues the cost chains.  ps carries the
 * ray arrays of the call (or of its gathered rays); its r0, r1, n, geom, rad, atm_time and `above` are set here.  The
 * model's view is left on the trial atmosphere.  Nothing is waited for after the stacking. */
/* hy.n > 0 (the hydrostatic balance is on): the segments of the trial copies, balanced after the elements have moved.
 * of (JUR_OVERFLOW_ISOLATE): the untraceable rays of every pass are flagged in of->flag (zeroed by the caller) before the
 * next pass overwrites the counts, and folded into the costs after the last. */
static int trial_run(jur_model_t *m, hipStream_t s, char const *who, atm_t const *atm, trial_dev_t *td, long nb, long npass,
                     long const *pass, long nmax, scene_fov_t *fv, jur_hyseg_t hy) {
  jur_scene_stack_t *const sk = &td->sk; jur_scene_trial_t *const st = &td->st; jur_scene_trial_pass_t *const ps = &td->ps;
  jur_scene_pquad_t const *const tq = td->tq.R ? &td->tq : NULL; jur_scene_ovfold_t const *const of = td->of.flag ? &td->of : NULL;
  size_t const nrow = (size_t)sk->nrow;
  int const nd = ps->nd;
  int rc;
  m->h_atm_n = 0;
  if ((rc = install_stacked_rows(m, atm, sk->nt, sk->ncopy - 1))) return rc;
  sk->rows = (double *)m->d_atm; st->rows = (double *)m->d_atm;
  int ti = scene_timed_begin(m, s);
  int ek = jurk_scene_stack(sk, s);
  if (!ek) ek = jurk_scene_elements(st, JUR_ELEM_APPLY, nb, s);
  if (hy.n > 0) {                                  /* (a timed launch of its own, between the two halves of this one) */
    scene_timed_end(m, ti, s);
    if (!ek) ek = scene_hydro_launch(m, s, hy, (double *)m->d_atm, (size_t)sk->nt);
    ti = scene_timed_begin(m, s);
  }
  hipError_t e = hipMemsetAsync(ps->cost, 0, sizeof(double) * (size_t)ps->nslice * (size_t)ps->ntrial, s);
  if (!ek && e == hipSuccess) {
    if (st->ivar) {
      ek = jurk_scene_prior(st, s);
      if (!ek && tq) {                              /* a full prior precision: + d^T R d, d = xa - (x + dx) in tq->v */
        jur_scene_trial_t dq = *st;
        dq.out = (double *)tq->v;
        ek = jurk_scene_prior_diff(&dq, nb, s);
        if (!ek) ek = jurk_scene_prior_quad(tq, s);
      }
    }
    else e = hipMemsetAsync(st->prior, 0, sizeof(double) * (size_t)ps->nslice * (size_t)ps->ntrial, s);
  }
  scene_timed_end(m, ti, s);
  if (!ek) ek = jurk_prepare_atm(&m->view, (double *)m->d_atm + nrow * (size_t)sk->nt, s);
  if (ek || e != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
    (void)hipGetLastError(); m->view.atm_np = 0; jur_set_error("%s: stacking the trial atmosphere failed", who); return JUR_EHIP;
  }
  if ((rc = jur_model_reserve(m, nmax))) return rc;
  ps->atm_time = m->view.atm_time;
  ps->above = sk->tmax + ((double)sk->ncopy + 1.0) * sk->span;
  for (long p = 0; p < npass; p++) {
    long const n = (pass[p + 1] - pass[p]) * ps->ntrial;
    size_t const N = (size_t)n;
    ps->r0 = pass[p]; ps->r1 = pass[p + 1]; ps->n = n;
    ps->geom = m->d_io; ps->rad = ps->geom + 7 * N;
    double *const tau = ps->rad + N * nd, *const tp = tau + N * nd;
    if (SCENE_TIMED(m, s, jurk_scene_trial_rays(ps, s))) return launch_failed("%s: trial replication kernel launch failed", who);
    if ((rc = jur_formod_device(m, n, ps->geom, ps->rad, tau, tp, m->d_io_np, m->d_status, s))) return rc;
    jur_scene_trial_pass_t pf = *ps;
    if (fv) {                                    /* the costs read the convolved radiances under the effective mask */
      fv->k.r0 = ps->r0; fv->k.r1 = ps->r1; fv->k.ntrial = ps->ntrial; fv->k.rowptr = NULL;
      fv->k.rad = ps->rad; fv->k.tau = NULL; fv->k.rad_f = m->d_fov; fv->k.tau_f = NULL;
      if (SCENE_TIMED(m, s, jurk_scene_fov(&fv->k, s))) return launch_failed("%s: field-of-view kernel launch failed", who);
      pf.rad = m->d_fov; pf.in_rad = fv->live;
    }
    if (SCENE_TIMED(m, s, jurk_scene_trial_cost(&pf, s))) return launch_failed("%s: trial cost kernel launch failed", who);
    if (of) {
      jur_scene_ovf_t oq;
      memset(&oq, 0, sizeof oq);
      oq.n = n; oq.r0 = ps->r0; oq.r1 = ps->r1; oq.ntrial = ps->ntrial; oq.per = ps->ntrial; oq.nslice = ps->nslice;
      oq.tcopy0 = ps->tcopy0; oq.np = m->d_io_np; oq.flag = (int *)of->flag;
      if (SCENE_TIMED(m, s, jurk_scene_overflow(&oq, s))) return launch_failed("%s: overflow kernel launch failed", who);
    }
  }
  if (of && SCENE_TIMED(m, s, jurk_scene_overflow_fold(of, s))) return launch_failed("%s: overflow fold kernel launch failed", who);
  return JUR_OK;
}

/* the refusals of jur_retrieve_scene_host that need no sizes */
static int retrieve_check_args(char const *who, jur_retrieve_in_t const *in, jur_retrieve_out_t const *out) {
  if (!in || !out) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  if (in->max_iter < 1) { jur_set_error("%s: max_iter = %d: at least one iteration is needed", who, in->max_iter); return JUR_EINVAL; }
  if (in->nlam < 1 || in->nlam > 8) { jur_set_error("%s: nlam = %d: 1 to 8 dampings per iteration", who, in->nlam); return JUR_EINVAL; }
  if (in->mode != JUR_DAMP_MARQUARDT && in->mode != JUR_DAMP_PRIOR) { jur_set_error("%s: unknown mode %d", who, in->mode); return JUR_EINVAL; }
  if (!in->fac) { jur_set_error("%s: null argument (fac)", who); return JUR_EINVAL; }
  int above_one = 0;
  for (int l = 0; l < in->nlam; l++) {
    if (!(in->fac[l] > 0) || isinf(in->fac[l])) { jur_set_error("%s: fac[%d] is %g: not positive or not finite", who, l, in->fac[l]); return JUR_EINVAL; }
    if (in->fac[l] > 1) above_one = 1;
  }
  if (!above_one) { jur_set_error("%s: no fac above 1: a rejected damping could never grow", who); return JUR_EINVAL; }
  if (!(in->lam_min > 0) || !(in->lam_min <= in->lam0) || !(in->lam0 <= in->lam_max) || isinf(in->lam_max)) {
    jur_set_error("%s: lam_min = %g, lam0 = %g, lam_max = %g: need 0 < lam_min <= lam0 <= lam_max, all finite", who, in->lam_min,
                  in->lam0, in->lam_max);
    return JUR_EINVAL;
  }
  if (!(in->tol >= 0) || isinf(in->tol)) { jur_set_error("%s: tol is %g: negative or not finite", who, in->tol); return JUR_EINVAL; }
  if (!in->prior_ivar != !in->prior_xa) {
    jur_set_error("%s: %s without %s: the prior is given as a pair", who, in->prior_ivar ? "prior_ivar" : "prior_xa",
                  in->prior_ivar ? "prior_xa" : "prior_ivar");
    return JUR_EINVAL;
  }
  if (in->mode == JUR_DAMP_PRIOR && !in->prior_ivar) { jur_set_error("%s: JUR_DAMP_PRIOR without a prior", who); return JUR_EINVAL; }
  if (!out->x || !out->lam || !out->cost || !out->prior || !out->nlive || !out->state || !out->iters) {
    jur_set_error("%s: null argument (%s)", who, !out->x ? "x" : !out->lam ? "lam" : !out->cost ? "cost" : !out->prior ? "prior" :
                  !out->nlive ? "nlive" : !out->state ? "state" : "iters");
    return JUR_EINVAL;
  }
  int const nh = !!out->h_cost + !!out->h_prior + !!out->h_lam + !!out->h_tcost + !!out->h_tprior + !!out->h_status + !!out->h_best +
                 !!out->h_accept + !!out->h_work;
  if (nh != 0 && nh != 9) { jur_set_error("%s: %d of the 9 history arrays are given: all or none", who, nh); return JUR_EINVAL; }
  return JUR_OK;
}

/* a diagonal prior laid out by wptr: r >= 0 and finite, xa finite */
static int prior_check_values(char const *who, long nslice, long const *wptr, double const *ivar, double const *xa) {
  for (long q = 0; q < nslice; q++)
    for (long e = wptr[q]; e < wptr[q + 1]; e++) {
      if (!(ivar[e] >= 0) || isinf(ivar[e])) {
        jur_set_error("%s: prior_ivar of slice %ld, element %ld is %g: negative or not finite", who, q, e - wptr[q], ivar[e]);
        return JUR_EINVAL;
      }
      if (!isfinite(xa[e])) {
        jur_set_error("%s: prior_xa of slice %ld, element %ld is %g: not finite", who, q, e - wptr[q], xa[e]);
        return JUR_EINVAL;
      }
    }
  return JUR_OK;
}

/* what jur_retrieve_scene_host adds to jur_step_scene_host */
typedef struct { jur_retrieve_in_t const *in; jur_retrieve_out_t const *out; atm_t *atm_ret; } scene_retrieve_t;
/* what jur_gradient_scene_host brings: the blocks of all rays, laid out by rowptr */
typedef struct { double const *k; } scene_grad_t;
/* what jur_param_scene_host brings to its two calls of the body.  Phase 1 is jur_gain_scene_host's, with the gain and the
 * effective weights written to the model's side buffer (gain, weff).  Phase 2 is jur_kernel_scene_host's under the
 * parameters' windows, where after the quotients of every pass the chains of C are continued: q holds the kernel's
 * arguments (all in the side buffer but kb, the blocks of the pass); wptr .. sid are the host's layout of the retrieved
 * state, mark and hmap its scratch for the tiles of a pass and d_pmap their place on the device.  bytes: the side buffer,
 * counted against the budget before the parts of the slab. */
typedef struct {
  int phase;
  size_t bytes;
  double *gain, *weff;
  jur_scene_param_t q;
  long const *wptr, *bwptr, *sptr;
  int const *srays, *sid;
  long *mark;
  int *hmap, *d_pmap;
} scene_param_t;

/* the tiles of C that the rays [r0, r1) of a pass reach, and the kernel on them; kb: the blocks of the pass, the first of
 * them kb0 doubles into the blocks of all rays.  The host's map is free again once the stream has been waited for. */
static int param_pass_extend(jur_model_t *m, hipStream_t s, char const *who, scene_param_t *pm, long r0, long r1, double const *kb, long kb0) {
  long const nt = jur_param_pass_maps(pm->wptr, pm->bwptr, pm->sptr, pm->srays, pm->sid, r0, r1, pm->mark, pm->hmap);
  if (nt == 0) return JUR_OK;
  hipError_t const e = hipMemcpyAsync(pm->d_pmap, pm->hmap, sizeof(int) * 5 * (size_t)nt, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); return JUR_EHIP; }
  pm->q.kb = kb;
  int const ti = scene_timed_begin(m, s);
  if (ti >= 0) m->evkind[ti] = 6;
  int const ek = jurk_scene_cross_pass(&pm->q, pm->d_pmap, nt, kb0, s);
  scene_timed_end(m, ti, s);
  if (ek) { jur_set_error("%s: cross-state kernel launch failed", who); return JUR_EHIP; }
  return JUR_OK;
}

/* ---- what jur_kernel_scene_host's family and jur_trial_scene_host open with ------------------------------------------- */
/* the atmosphere a scene entry can take: no global balance (hydz_tail: why not, in the entry's words), 2..JUR_NP points,
 * ascending time stamps */
/* The scene entries are built on per-ray blocks of ONE slice's state; under ip == 2 a ray reads two profiles of a track.
 * Refused before anything else is looked at. */
static int scene_ip_check(jur_model_t const *m, char const *who) {
  if (m->ctl->ip == 3) {
    jur_set_error("%s: ip = 3 (point cloud) averages every point of a ray over the air parcels around it, and the scene entries "
                  "hold the state of one slice per ray: use jur_formod_host and jur_kernel", who);
    return JUR_EINVAL;
  }
  if (m->ctl->ip != 2) return JUR_OK;
  jur_set_error("%s: ip = 2 (satellite track) interpolates every point of a ray between two profiles, and the scene entries "
                "hold the state of one slice per ray: use jur_formod_host and jur_kernel", who);
  return JUR_EINVAL;
}

static int scene_atm_check(jur_model_t const *m, char const *who, char const *hydz_tail, atm_t const *atm) {
  if (m->ctl->hydz >= 0) {
    jur_set_error("%s: hydz = %g >= 0 adjusts all points as one profile, so %s", who, m->ctl->hydz, hydz_tail);
    return JUR_EINVAL;
  }
  if (atm->np < 2 || atm->np > JUR_NP) { jur_set_error("%s: need 2..%d atmospheric points", who, JUR_NP); return JUR_EINVAL; }
  for (int i = 1; i < atm->np; i++)
    if (!(atm->time[i] >= atm->time[i - 1])) {
      jur_set_error("%s: the time stamps of the atmosphere are not ascending (point %d): the slices of a "
                    "stacked atmosphere cannot reproduce locate_atm there", who, i);
      return JUR_EINVAL;
    }
  return JUR_OK;
}

/* The host products of a call's rays and atmosphere, before the entries diverge: the slice of every ray (first | len,
 * and behind them nr ints that are the caller's), jur_scene_layout's rowptr, the distinct slices with state elements
 * and the slice of every ray (sid), the ray slices of the hydrostatic balance (hyf: first | len, nrs of them; balance on),
 * the effective mask of a field of view (hlive; one is set), the base rows with their stacked time stamps, and the
 * largest time stamp and the span of atmosphere and rays together. */
typedef struct {
  int *first, *len, *sid, *hyf;
  long *rp, nslice, nrs;
  jur_scene_slice_t *sl;
  double *hlive, *hbase, tmax, span;
} scene_open_t;

static void scene_open_free(scene_open_t *o) {
  free(o->first); free(o->rp); free(o->sid); free(o->sl); free(o->hyf); free(o->hlive); free(o->hbase);
  memset(o, 0, sizeof *o);
}

/* no_k: the refusal of a state that has elements, where the caller has brought no array for its blocks; sums: the sums
 * over the rays are formed, so y is needed and the weights are checked.  On an error the caller frees what stands. */
static int scene_open(scene_open_t *o, jur_model_t *m, char const *who, atm_t const *atm, long nr, double const *const geom[7],
                      double const *rad_in, long const *rowptr, char const *no_k, int sums, double const *y, double const *weight) {
  int const np0 = atm->np, nd = m->ctl->nd;
  size_t const NR = (size_t)nr, nrow = 6 + (size_t)m->view.ng + m->view.nw;
  int rc;
  memset(o, 0, sizeof *o);
  o->first = (int *)malloc(sizeof(int) * 3 * NR);
  o->rp = (long *)malloc(sizeof(long) * (NR + 1));
  o->sid = (int *)malloc(sizeof(int) * NR);
  if (!o->first || !o->rp || !o->sid) return JUR_ENOMEM;
  o->len = o->first + NR;
  if ((rc = jur_scene_layout(m->ctl, atm, nr, geom[0], o->first, o->len, o->rp))) return rc;
  if (memcmp(o->rp, rowptr, sizeof(long) * (NR + 1))) {
    jur_set_error("%s: rowptr is not jur_scene_layout's for these rays, this atmosphere and these windows", who);
    return JUR_EINVAL;
  }
  if (o->rp[nr] > 0 && no_k) { jur_set_error(no_k, who); return JUR_EINVAL; }
  if (sums) {
    if (!y || !weight) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
    for (long r = 0; r < nr; r++)
      for (int id = 0; id < nd; id++) {
        double const w = weight[(size_t)r * nd + id];
        if (!(w >= 0) || isinf(w)) {
          jur_set_error("%s: the weight of ray %ld, channel %d is %g: negative or not finite", who, r, id, w);
          return JUR_EINVAL;
        }
      }
  }
  if (m->fov_n > 0 && (rc = scene_fov_mask(who, nd, nr, geom[0], rad_in, &o->hlive))) return rc;
  if (m->scene_hydz >= 0) {                         /* the slices the rays are traced through, with or without elements */
    if (!(o->hyf = (int *)malloc(sizeof(int) * 2 * NR))) return JUR_ENOMEM;
    if ((o->nrs = jur_scene_ray_slices_of(np0, nr, o->first, o->len, o->hyf, o->hyf + NR)) < 0) return JUR_ENOMEM;
    if ((rc = jur_scene_hydro_check(who, np0, o->nrs, o->hyf, o->hyf + NR))) return rc;
  }
  /* the distinct slices that have state elements, in the order the rays meet them */
  if ((o->nslice = jur_scene_distinct(np0, nr, o->first, o->len, o->rp, o->sid, &o->sl)) < 0) return JUR_ENOMEM;
  if (!(o->hbase = (double *)malloc(sizeof(double) * nrow * (size_t)np0))) return JUR_ENOMEM;
  pack_atm_rows(m, atm, o->hbase, (size_t)np0, 0);
  stack_times(o->hbase, atm->time, np0, 0.0);
  double tmin = atm->time[0];
  o->tmax = atm->time[0];
  for (int i = 0; i < np0; i++) { tmin = fmin(tmin, atm->time[i]); o->tmax = fmax(o->tmax, atm->time[i]); }
  for (long i = 0; i < nr; i++) { tmin = fmin(tmin, geom[0][i]); o->tmax = fmax(o->tmax, geom[0][i]); }
  o->span = (o->tmax - tmin) + 1.0;
  return JUR_OK;
}

/* The uploads a call opens with, enqueued on s, to where the caller's slab has them: the base rows, the 7 geometry rows,
 * the input radiances, nfl * nr ints of first | len (| the caller's own), the zeroed status word and, where a field of view
 * is set, the effective mask.  fv is filled for the rays of the call. */
static hipError_t scene_open_upload(jur_model_t *m, hipStream_t s, scene_open_t const *o, int np0, long nr, double const *const geom[7],
                                    double const *rad_in, double *d_base, double *d_geom, double *d_inrad, int *d_first, int nfl,
                                    double *d_live, scene_fov_t *fv) {
  size_t const NR = (size_t)nr, nrow = 6 + (size_t)m->view.ng + m->view.nw, nrd = NR * (size_t)m->ctl->nd;
  hipError_t e = hipMemcpyAsync(d_base, o->hbase, sizeof(double) * nrow * (size_t)np0, hipMemcpyHostToDevice, s);
  for (int q = 0; q < 7 && e == hipSuccess; q++) e = hipMemcpyAsync(d_geom + (size_t)q * NR, geom[q], sizeof(double) * NR, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_inrad, rad_in, sizeof(double) * nrd, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_first, o->first, sizeof(int) * (size_t)nfl * NR, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(m->d_status, 0, sizeof(int), s);
  if (m->fov_n > 0 && e == hipSuccess) e = hipMemcpyAsync(d_live, o->hlive, sizeof(double) * nrd, hipMemcpyHostToDevice, s);
  memset(fv, 0, sizeof *fv);
  fv->k.nr = nr; fv->k.nd = m->ctl->nd; fv->k.time = d_geom; fv->k.vpz = d_geom + 4 * NR;
  fv->k.n = m->fov_n; fv->k.dz = m->d_fov_shape; fv->k.w = m->d_fov_shape + JUR_NSHAPE; fv->k.status = m->d_status;
  fv->live = d_live;
  return e;
}

/* A cut of a call's rays into passes: pass p is the rays [cut[p], cut[p + 1]) of the rays that rp (host) is the rowptr of.
 * fwd: forward-only passes, one slot per ray and no blocks (the pass view comes with the all-zero rowptr then).  stay: the
 * blocks of a Jacobian pass are written where they lie among those of all rays, from k on (device), not over those of
 * the pass before.  k_home: where the blocks go on the host, or NULL. */
typedef struct { long const *cut; long n; long const *rp; int fwd, stay; double *k, *k_home; } scene_cut_t;

/* JUR_OVERFLOW_ISOLATE in the passes of a retrieval's iteration: the untraceable slots of every pass are flagged in
 * fold.flag (the slice of a ray from tcopy0 and per, as jur_scene_ovf_t's), before the next pass overwrites the counts;
 * after the last pass the flagged slices fail, on the device */
typedef struct { int per; int const *tcopy0; jur_scene_ovfold_t fold; } scene_ovflags_t;

/* The passes of one cut over the stacked atmosphere.  Installs and stacks the rows (st), balances the raised copies (hy),
 * prepares the atmosphere, waits once and reserves the forward model's workspace for the largest pass, nmax slots.  Then
 * per pass: the rays are replicated, the forward model runs, the untraceable slots are flagged (ov), the results are
 * convolved (fv), the quotients taken, the sums continued (nq over ntiles tiles; forward-only from the held blocks gq over
 * ngroups workgroups) and the chains of C (pm: phase 2 of jur_param_scene_host), the blocks go home, and the pass is
 * waited for.  a carries the ray arrays and the rowptr of the cut's rays; what belongs to a pass is set here. */
static int scene_passes_run(jur_model_t *m, hipStream_t s, char const *who, atm_t const *atm, jur_scene_stack_t *st, jur_scene_pass_t *a,
                            jur_scene_normal_t const *nq, long ntiles, jur_scene_grad_t const *gq, long ngroups, scene_fov_t *fv,
                            jur_hyseg_t hy, scene_cut_t const *c, scene_ovflags_t const *ov, scene_param_t *pm, long nmax) {
  int const nd = a->nd, fwd = c->fwd;
  long const *const rp = c->rp;
  int rc;
  m->h_atm_n = 0;                                /* the device no longer holds the caller's atmosphere */
  if ((rc = install_stacked_rows(m, atm, st->nt, st->ncopy - 1))) return rc;
  st->rows = (double *)m->d_atm;
  a->atm_time = m->view.atm_time;
  int ek = SCENE_TIMED(m, s, jurk_scene_stack(st, s));
  if (!ek) ek = scene_hydro_launch(m, s, hy, (double *)m->d_atm, (size_t)st->nt);
  if (!ek) ek = jurk_prepare_atm(&m->view, (double *)m->d_atm + (size_t)st->nrow * (size_t)st->nt, s);
  /* the one wait before the passes: the uploads have left the host arrays, the stacked rows stand */
  if (ek || hipStreamSynchronize(s) != hipSuccess) {
    (void)hipGetLastError(); m->view.atm_np = 0; jur_set_error("%s: stacking the atmosphere failed", who); return JUR_EHIP;
  }
  if ((rc = jur_model_reserve(m, nmax))) return rc;   /* the forward model's workspace for the largest pass, before the first */
  for (long p = 0; p < c->n; p++) {
    long const r0 = c->cut[p], r1 = c->cut[p + 1], n = fwd ? r1 - r0 : (rp[r1] - rp[r0]) + (r1 - r0), nk = fwd ? 0 : (rp[r1] - rp[r0]) * nd;
    size_t const N = (size_t)n;
    a->r0 = r0; a->r1 = r1; a->n = n;
    if (c->stay && !fwd) a->k = c->k + (size_t)rp[r0] * (size_t)nd;
    a->geom = m->d_io; a->rad = a->geom + 7 * N; a->tau = a->rad + N * nd; a->tp = a->tau + N * nd; a->np = m->d_io_np;
    if (SCENE_TIMED(m, s, jurk_scene_rays(a, s))) return launch_failed("%s: replication kernel launch failed", who);
    if ((rc = jur_formod_device(m, n, a->geom, a->rad, a->tau, a->tp, a->np, m->d_status, s))) return rc;
    if (ov) {
      jur_scene_ovf_t oq;
      memset(&oq, 0, sizeof oq);
      oq.n = n; oq.r0 = r0; oq.r1 = r1; oq.ntrial = 0; oq.per = ov->per; oq.nslice = ov->fold.nslice;
      oq.rowptr = a->rowptr; oq.tcopy0 = ov->tcopy0; oq.np = a->np; oq.flag = (int *)ov->fold.flag;
      if (SCENE_TIMED(m, s, jurk_scene_overflow(&oq, s))) return launch_failed("%s: overflow kernel launch failed", who);
    }
    jur_scene_pass_t af = *a;                    /* what reads the forward model's results ... */
    if (fv) {                                    /* ... reads them convolved, the sums under the effective mask */
      fv->k.r0 = r0; fv->k.r1 = r1; fv->k.ntrial = 0; fv->k.rowptr = a->rowptr;
      fv->k.rad = a->rad; fv->k.tau = a->tau; fv->k.rad_f = m->d_fov; fv->k.tau_f = fv->tau;
      if (SCENE_TIMED(m, s, jurk_scene_fov(&fv->k, s))) return launch_failed("%s: field-of-view kernel launch failed", who);
      af.rad = m->d_fov; af.fov_tau = fv->tau; af.in_rad = fv->live;
    }
    if (SCENE_TIMED(m, s, jurk_scene_quot(&af, nk, s))) return launch_failed("%s: quotient kernel launch failed", who);
    if (ntiles && !fwd && SCENE_TIMED(m, s, jurk_scene_normal(&af, nq, ntiles, s))) return launch_failed("%s: normal-equation kernel launch failed", who);
    if (ngroups && fwd && SCENE_TIMED(m, s, jurk_scene_gradient(&af, nq, gq, ngroups, s))) return launch_failed("%s: gradient kernel launch failed", who);
    if (pm && (rc = param_pass_extend(m, s, who, pm, r0, r1, a->k, rp[r0] * nd))) return rc;
    /* the blocks of the pass go home (where asked for); the one wait of the pass */
    hipError_t e = (nk > 0 && c->k_home) ? hipMemcpyAsync(c->k_home + (size_t)rp[r0] * nd, a->k, sizeof(double) * (size_t)nk, hipMemcpyDeviceToHost, s) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); return JUR_EHIP; }
  }
  /* all passes are done: the flagged slices fail before the solve */
  if (ov && SCENE_TIMED(m, s, jurk_scene_overflow_fold(&ov->fold, s))) return launch_failed("%s: overflow fold kernel launch failed", who);
  return JUR_OK;
}

/* The loop's part of the slab (jur_retrieve_scene_host).  dbl doubles: tcost | tprior [nlam][ns] | prior0 [ns] | xout | xa
 * [nb] | the arrays of the rays that remain once slices have ended: geom [7][nr] | rad | y | weight [nr][nd] | dvec, xa - (x
 * + dx) of every trial [nlam][nb] (a full prior precision) | box, lo | hi [nb] (the state is bounded).  lng longs behind
 * them: the plan's | rowptr [nr + 1] and sptr [ns + 1] of the rays that remain | ov_lng partial counts of the two folds.
 * ints, among the slab's: the plan's | state | choice [ns] | act | first | len | copy0 | tcopy0 of the rays that remain [nr]
 * | their srays [nlist] | ov_int flags of the slices [ns] and of the trials [nlam][ns] (JUR_OVERFLOW_ISOLATE). */
typedef struct { size_t dvec, box, ov_int, ov_lng, dbl, lng, ints; } loop_layout_t;

static loop_layout_t loop_layout(trial_plan_t const *pl, size_t nr, size_t nrd, int full, int isolate) {
  size_t const RL = (size_t)pl->ntrial, RS = (size_t)pl->nslice, nb = (size_t)pl->nb;
  loop_layout_t o;
  o.dvec = full ? RL * nb : 0; o.box = pl->box ? 2 * nb : 0;
  o.ov_int = isolate ? RS + RL * RS : 0; o.ov_lng = isolate ? 2 * (size_t)JUR_OVERFLOW_PARTS : 0;
  o.dbl = 2 * RL * RS + RS + 2 * nb + 7 * nr + 3 * nrd + o.dvec + o.box;
  o.lng = pl->nlong + (nr + 1) + (RS + 1) + o.ov_lng;
  o.ints = pl->nint + 2 * RS + 5 * nr + (size_t)pl->nlist + o.ov_int;
  return o;
}

/* once slices have ended: the views of both kinds of pass read the rays that cq has gathered, rpc | sptrc | sraysc their
 * rowptr and lists */
static void scene_views_gathered(jur_scene_compact_t const *cq, long const *rpc, long const *sptrc, int const *sraysc, trial_dev_t *td,
                                 jur_scene_pass_t *a, jur_scene_normal_t *nq, scene_fov_t *fv) {
  jur_scene_trial_pass_t *const ps = &td->ps;
  a->nr = ps->nr = fv->k.nr = cq->n;
  a->rowptr = rpc;
  a->first = ps->first = cq->first_c; a->len = ps->len = cq->len_c; a->copy0 = cq->copy0_c; ps->tcopy0 = cq->tcopy0_c;
  a->in_geom = ps->in_geom = fv->k.time = cq->geom_c; fv->k.vpz = cq->geom_c + 4 * cq->n;
  a->in_rad = ps->in_rad = cq->rad_c;
  nq->sptr = ps->sptr = sptrc; nq->srays = ps->srays = sraysc;
  nq->y = ps->y = cq->y_c; nq->weight = ps->weight = cq->weight_c;
  fv->live = cq->live_c;
}

/* jur_retrieve_scene_host behind the opening: the iterations, each the passes of a Jacobian or reuse iteration, the solve
 * for every damping, the trial pass on the steps where they lie and the policy; then the forward model on the retrieved
 * atmosphere, *ret_atm (malloc'ed), whose results a->out_* name.  The views st, a, nq, gq and fv come as the opening has
 * filled them for all rays of the call; d_base: the base rows.  ntiles == 0: no state elements, nothing to retrieve.
 * scan_time: the time stamps of the rays.  The slab's parts are the caller's: Wrc (all-zero rowptr | koff | gptr of the held blocks, hkoff the host's; with
 * kernel_recomp > 1), Wsv (solve_layout), Wrt and Irt (loop_layout), Wfov (a field of view: the mask of the rays that
 * remain | the convolved radiances of the last forward model); hy: the balance's segments of the ray slices | the raised
 * copies | the trial copies.  pass: the three cuts (Jacobian | trial | forward-only passes, nr + 1 longs each) as first
 * made, cut anew here within cap and nmax once slices have ended. */
static int retrieve_loop(jur_model_t *m, hipStream_t s, char const *who, atm_t const *atm, long nr, double const *scan_time,
                         scene_retrieve_t const *rt, scene_open_t const *op, trial_plan_t const *pl, long ntiles, long na, long cap,
                         long nmax, long *pass, long npass, long ntpass, long nfpass, jur_scene_stack_t *st, jur_scene_pass_t *a,
                         jur_scene_normal_t *nq, jur_scene_grad_t const *gq, scene_fov_t *fv, double *d_base, long *Wrc, long *hkoff,
                         jur_hyseg_t const hy[3], double const *d_R, double *Wsv, double *Wrt, int *Irt, double *Wfov, atm_t **ret_atm) {
  jur_retrieve_in_t const *const rin = rt->in;
  jur_retrieve_out_t const *const ro = rt->out;
  int const looping = ntiles > 0, np0 = atm->np, nd = a->nd, fov = m->fov_n > 0, hyd = m->scene_hydz >= 0;
  int const ov = m->scene_overflow == JUR_OVERFLOW_ISOLATE, ovl = ov && looping;   /* untraceable rays fail their trial or their slice, not the call */
  int const every = looping ? m->kernel_recomp : 1;
  long const nslice = op->nslice, nb = pl->nb, *const rp = op->rp;
  int const *const sid = op->sid;
  size_t const NR = (size_t)nr, nrd = NR * (size_t)nd, RL = (size_t)rin->nlam, RS = (size_t)nslice, nacc = (size_t)na + (size_t)nb + 2 * RS;
  double const *const d_geom = a->in_geom, *const d_inrad = a->in_rad;   /* (of all rays: the views move on to the rays that remain) */
  double *const d_k = a->k;
  long const ngroups = every > 1 ? hkoff[NR + RS] : 0;   /* (hkoff: koff [nr] | gptr [ns + 1]) */
  long *const tpass = pass + NR + 1, *const fpass = tpass + NR + 1, *const d_zrp = Wrc, *const d_koff = Wrc + NR + 1;
  int rc = JUR_OK; hipError_t e = hipSuccess;
  /* host arrays of the loop.  rd: lamt | pred | tcost | tprior | Jt [nlam][ns] each, cost | prior | J [ns] each; ri: status
   * [nlam][ns], best | accept | choice [ns] each; hov: what comes home of the overflow flags per iteration, state [ns] |
   * trial flags [nlam][ns], hovp the folds' partial counts; hjac: the states at the last Jacobian iteration */
  double *rd = (double *)calloc(5 * RL * RS + 3 * RS + 1, sizeof(double)), *htimec = NULL;
  int *ri = (int *)calloc(RL * RS + 4 * RS + 1, sizeof(int)), *hact = NULL, *hov = NULL, *hjac = NULL;
  long *hcomp = NULL, *hovp = NULL; atm_t *ret = NULL;
  if (!rd || !ri) { rc = JUR_ENOMEM; goto done; }
  double *const lamt = rd, *const htcost = rd + 2 * RL * RS, *const htprior = rd + 3 * RL * RS, *const Jt = rd + 4 * RL * RS,
         *const hcost = rd + 5 * RL * RS, *const hprior0 = hcost + RS, *const J = hprior0 + RS;
  int *const hstatus = ri, *const best = ri + RL * RS, *const accept = best + RS, *const choice = accept + RS;
  /* the dampings, predictions and statuses of an iteration as solve_enqueue takes them: the prior pair is on the device */
  jur_solve_in_t const sin = {.nlam = rin->nlam, .mode = rin->mode, .lam = lamt, .prior_ivar = rin->prior_ivar, .prior_dx = rin->prior_xa};
  jur_solve_out_t const sout = {.pred = rd + RL * RS, .status = hstatus};

  /* the loop's part of the slab, the solver's part where the loop reads it */
  loop_layout_t const ll = loop_layout(pl, NR, nrd, d_R != NULL, ov);
  solve_layout_t const svl = solve_layout((size_t)na, (size_t)nb, RS, RL, rin->prior_ivar != NULL, d_R != NULL);
  double *const d_tcost = Wrt, *const d_tprior = d_tcost + RL * RS, *const d_prior0 = d_tprior + RL * RS, *const d_xout = d_prior0 + RS,
         *const d_xa = d_xout + nb, *const d_geomc = d_xa + nb, *const d_radc = d_geomc + 7 * NR, *const d_yc = d_radc + nrd,
         *const d_wc = d_yc + nrd, *const d_dvec = d_wc + nrd, *const d_bd = d_dvec + ll.dvec;
  long *const Lr = (long *)(Wrt + ll.dbl), *const d_rpc = Lr + pl->nlong, *const d_sptrc = d_rpc + NR + 1, *const d_ovp = d_sptrc + RS + 1;
  int *const Ir = Irt, *const d_state = Ir + pl->nint, *const d_choice = d_state + RS, *const d_act = d_choice + RS,
      *const d_firstc = d_act + NR, *const d_lenc = d_firstc + NR, *const d_copy0c = d_lenc + NR, *const d_tcopy0c = d_copy0c + NR,
      *const d_sraysc = d_tcopy0c + NR, *const d_oflag = d_sraysc + pl->nlist, *const d_otflag = d_oflag + RS;
  double *const d_livec = Wfov, *const d_frad = Wfov + nrd;
  double *const sv_dx = Wsv + svl.dx, *const sv_r = Wsv + svl.r, *const sv_d = Wsv + svl.d;
  long const novj = jur_scene_overflow_parts((long)RS), novt = jur_scene_overflow_parts((long)(RL * RS));
  size_t const npr = (looping && rin->prior_ivar) ? (size_t)nb : 0;
  trial_dev_t td;
  scene_ovflags_t ovj;
  jur_scene_compact_t cq;                         /* the gather: from the arrays of all rays into the loop's */
  memset(&td, 0, sizeof td); memset(&ovj, 0, sizeof ovj); memset(&cq, 0, sizeof cq);
  long *hrpc = NULL, *hsptrc = NULL, *hnlive = NULL;
  long const *rp_cur = rp, *d_rp_cur = a->rowptr;   /* rowptr of the rays of a Jacobian pass: of all rays, or of those that remain */
  long nr_cur = nr, nactive_built = (pl->nlist == nr) ? nslice : -1;   /* (rays without state elements are in no pass of the loop) */
  double fac_max = 0;
  if (!looping) {                                 /* no state elements: nothing to retrieve */
    for (int it = 0; ro->h_work && it < rin->max_iter; it++) ro->h_work[2 * it] = ro->h_work[2 * it + 1] = 0;
  } else {
    hcomp = (long *)malloc(sizeof(long) * ((NR + 1) + (RS + 1) + RS));
    hact = (int *)malloc(sizeof(int) * (2 * NR + (size_t)pl->nlist + 1));
    if (every > 1) hjac = (int *)malloc(sizeof(int) * (RS + 1));
    if (!hcomp || !hact || (every > 1 && !hjac)) { rc = JUR_ENOMEM; goto done; }
    hrpc = hcomp; hsptrc = hrpc + NR + 1; hnlive = hsptrc + RS + 1;
    e = hipMemcpyAsync(Lr, pl->longs, sizeof(long) * pl->nlong, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(Ir, pl->ints, sizeof(int) * pl->nint, hipMemcpyHostToDevice, s);
    if (npr && e == hipSuccess) e = hipMemcpyAsync(sv_r, rin->prior_ivar, sizeof(double) * npr, hipMemcpyHostToDevice, s);
    if (npr && e == hipSuccess) e = hipMemcpyAsync(d_xa, rin->prior_xa, sizeof(double) * npr, hipMemcpyHostToDevice, s);
    if (ll.box && e == hipSuccess) e = hipMemcpyAsync(d_bd, pl->box, sizeof(double) * ll.box, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
    /* (tq: d^T R d of the loop's states: of the trials, of the state as it stands) */
    trial_dev_fill(&td, m, pl, np0, st->tmax, st->span, Lr, Ir, d_base, d_geom, d_inrad, a->first, a->len, nq->y, nq->weight, sv_dx,
                   npr ? sv_r : NULL, npr ? d_xa : NULL, d_tprior, d_tcost, ll.box ? d_bd : NULL, d_R, nq->aptr, d_dvec,
                   ovl ? d_otflag : NULL, d_ovp + JUR_OVERFLOW_PARTS, d_state, d_choice);
    cq.nr = nr; cq.nd = nd; cq.act = d_act;
    cq.geom = d_geom; cq.rad = d_inrad; cq.y = nq->y; cq.weight = nq->weight;
    cq.first = a->first; cq.len = a->len; cq.copy0 = a->copy0; cq.tcopy0 = td.ps.tcopy0;
    cq.geom_c = d_geomc; cq.rad_c = d_radc; cq.y_c = d_yc; cq.weight_c = d_wc;
    cq.first_c = d_firstc; cq.len_c = d_lenc; cq.copy0_c = d_copy0c; cq.tcopy0_c = d_tcopy0c;
    if (fov) { cq.live = fv->live; cq.live_c = d_livec; }
    if (ovl) {
      hov = (int *)malloc(sizeof(int) * (RS + RL * RS));
      hovp = (long *)malloc(sizeof(long) * 2 * JUR_OVERFLOW_PARTS);
      if (!hov || !hovp) { rc = JUR_ENOMEM; goto done; }
      ovj.per = rin->nlam; ovj.tcopy0 = td.ps.tcopy0;
      ovj.fold.nslice = nslice; ovj.fold.ntrial = 1; ovj.fold.flag = d_oflag; ovj.fold.state = d_state; ovj.fold.part = d_ovp;
    }
    for (int l = 0; l < rin->nlam; l++) fac_max = fmax(fac_max, rin->fac[l]);
    for (long q = 0; q < nslice; q++) { ro->lam[q] = rin->lam0; ro->state[q] = JUR_RET_ACTIVE; ro->iters[q] = 0; ro->cost[q] = ro->prior[q] = 0; ro->nlive[q] = 0; }
    if (ro->h_cost) {
      size_t const MI = (size_t)rin->max_iter;
      for (size_t i = 0; i < MI * RL * RS; i++) { ro->h_lam[i] = ro->h_tcost[i] = ro->h_tprior[i] = NAN; ro->h_status[i] = -1; }
      for (size_t i = 0; i < MI * RS; i++) ro->h_best[i] = ro->h_accept[i] = -1;
      for (size_t i = 0; i < 2 * MI; i++) ro->h_work[i] = 0;
    }
  }
  for (int it = 0; looping && it < rin->max_iter; it++) {
    /* the rays of the slices that are still active, in arrays of their own once a slice has ended */
    long nactive = 0;
    for (long q = 0; q < nslice; q++) nactive += ro->state[q] == JUR_RET_ACTIVE;
    if (nactive == 0) break;
    int const reuse = every > 1 && it % every != 0;   /* a reuse iteration */
    int regathered = 0;                             /* the rays were gathered anew in this iteration */
    if (nactive != nactive_built) {
      int *const act = hact, *const pos = hact + NR, *const sraysc = pos + NR;
      long const n = jur_scene_gather_active(nr, nslice, rp, sid, ro->state, pl->sptr, pl->srays, act, pos, hrpc, hsptrc, sraysc);
      long const nl = hsptrc[nslice];
      nr_cur = n; rp_cur = hrpc; nactive_built = nactive;
      if (fov) {                                    /* (whole scans have left: the scans that remain are the call's) */
        if (!htimec && !(htimec = (double *)malloc(sizeof(double) * NR))) { rc = JUR_ENOMEM; goto done; }
        for (long i = 0; i < n; i++) htimec[i] = scan_time[act[i]];
      }
      npass = jur_scene_passes(nr_cur, rp_cur, cap, fov ? htimec : NULL, pass, NULL, NULL);   /* (within nmax, kmax: jur_scene_pass_reserve) */
      ntpass = jur_trial_passes(nr_cur, rin->nlam, cap, fov ? htimec : NULL, tpass, NULL);
      if (every > 1) {
        long fmax = 0;
        nfpass = jur_trial_passes(nr_cur, 1, cap, fov ? htimec : NULL, fpass, &fmax);
        if (nfpass < 0 || fmax > nmax) { jur_set_error("%s: a forward-only pass of %ld slots, %ld reserved", who, fmax, nmax); rc = JUR_EINVAL; goto done; }
      }
      regathered = 1;
      e = hipMemcpyAsync(d_act, act, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s);
      if (e == hipSuccess) e = hipMemcpyAsync(d_sraysc, sraysc, sizeof(int) * (size_t)(nl ? nl : 1), hipMemcpyHostToDevice, s);
      if (e == hipSuccess) e = hipMemcpyAsync(d_rpc, hrpc, sizeof(long) * ((size_t)n + 1), hipMemcpyHostToDevice, s);
      if (e == hipSuccess) e = hipMemcpyAsync(d_sptrc, hsptrc, sizeof(long) * (RS + 1), hipMemcpyHostToDevice, s);
      if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
      cq.n = n;
      if (SCENE_TIMED(m, s, jurk_scene_compact(&cq, s))) { rc = launch_failed("%s: gathering kernel launch failed", who); goto done; }
      scene_views_gathered(&cq, d_rpc, d_sptrc, d_sraysc, &td, a, nq, fv);
      d_rp_cur = d_rpc; ovj.tcopy0 = td.ps.tcopy0;
    }
    /* the dampings of this iteration (the product is rounded first), the states, fresh accumulators, the prior */
    for (int l = 0; l < rin->nlam; l++)
      for (long q = 0; q < nslice; q++) {
        double const v = ro->lam[q] * rin->fac[l];
        lamt[(size_t)l * RS + (size_t)q] = fmin(fmax(v, rin->lam_min), rin->lam_max);
      }
    e = hipMemcpyAsync(d_state, ro->state, sizeof(int) * RS, hipMemcpyHostToDevice, s);
    if (ovl && e == hipSuccess) e = hipMemsetAsync(d_oflag, 0, sizeof(int) * ll.ov_int, s);
    /* (a reuse iteration keeps A of the last Jacobian iteration: b, cost and nlive alone start again) */
    if (it > 0 && e == hipSuccess) e = reuse ? hipMemsetAsync(nq->b, 0, sizeof(double) * (nacc - (size_t)na), s)
                                             : hipMemsetAsync(nq->A, 0, sizeof(double) * nacc, s);
    if (every > 1 && (!reuse || regathered)) {
      /* where the blocks of the rays that remain lie: a Jacobian iteration writes those of its rays back to back */
      if (!reuse) memcpy(hjac, ro->state, sizeof(int) * RS);
      long const nk = jur_scene_recomp_offsets(nr, rp, sid, hjac, ro->state, nd, hkoff);
      if (nk != nr_cur) { if (nk >= 0) jur_set_error("%s: retained blocks out of step", who); rc = JUR_EINVAL; goto done; }
      if (e == hipSuccess) e = hipMemcpyAsync(d_koff, hkoff, sizeof(long) * (size_t)nk, hipMemcpyHostToDevice, s);
    }
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
    int ek = 0;
    if (npr) {
      jur_scene_trial_t pq = td.st;
      pq.out = sv_d; pq.dx = NULL; pq.prior = d_prior0;
      int const ti = scene_timed_begin(m, s);
      ek = jurk_scene_elements(&pq, JUR_ELEM_PRIOR_DX, nb, s);
      if (!ek) ek = jurk_scene_prior(&pq, s);
      if (!ek && d_R) {                             /* (sv_d holds xa - x) */
        jur_scene_pquad_t bq = td.tq;
        bq.nvec = 1; bq.v = sv_d; bq.out = d_prior0;
        ek = jurk_scene_prior_quad(&bq, s);
      }
      scene_timed_end(m, ti, s);
    } else if (hipMemsetAsync(d_prior0, 0, sizeof(double) * RS, s) != hipSuccess) ek = 1;
    if (ek) { (void)hipGetLastError(); jur_set_error("%s: prior kernel launch failed", who); rc = JUR_EHIP; goto done; }

    /* the passes: a reuse iteration's are forward-only, one slot per ray, which the kernels of a pass make of the all-zero
     * rowptr; the blocks of a Jacobian iteration stay for them */
    scene_cut_t const cut = {reuse ? fpass : pass, reuse ? nfpass : npass, rp_cur, reuse, every > 1, d_k, NULL};
    a->rowptr = reuse ? d_zrp : d_rp_cur;
    if ((rc = scene_passes_run(m, s, who, atm, st, a, nq, ntiles, gq, ngroups, fov ? fv : NULL, hy[1], &cut,
                               ovl ? &ovj : NULL, NULL, nmax))) goto done;
    if ((rc = solve_enqueue(m, s, who, nslice, na, nb, nq->wptr, nq->aptr, nq->A, nq->b, Wsv, &sin, &sout, d_state, d_R))) goto done;

    /* the trial pass on the steps where they lie; the scalars of the iteration come home; the policy; the choices go up */
    if ((rc = trial_run(m, s, who, atm, &td, nb, ntpass, tpass, nmax, fov ? fv : NULL, hy[2]))) goto done;
    e = hipMemcpyAsync(hcost, nq->cost, sizeof(double) * RS, hipMemcpyDeviceToHost, s);
    if (ovl) {                                     /* the states and the trial flags come home with the scalars */
      if (e == hipSuccess) e = hipMemcpyAsync(hov, d_state, sizeof(int) * RS, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipMemcpyAsync(hov + RS, d_otflag, sizeof(int) * RL * RS, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipMemcpyAsync(hovp, d_ovp, sizeof(long) * (size_t)novj, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipMemcpyAsync(hovp + JUR_OVERFLOW_PARTS, d_ovp + JUR_OVERFLOW_PARTS, sizeof(long) * (size_t)novt, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(hnlive, nq->nlive, sizeof(long) * RS, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(hprior0, d_prior0, sizeof(double) * RS, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(htcost, d_tcost, sizeof(double) * RL * RS, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(htprior, d_tprior, sizeof(double) * RL * RS, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m->h_status, m->d_status, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
    if ((rc = scene_status_rc(m, who, ov))) goto done;
    if (ovl) {
      /* a slice that failed in this iteration took no part in it: what it holds is of its last completed iteration */
      for (long q = 0; q < nslice; q++)
        if (ro->state[q] == JUR_RET_ACTIVE && hov[q] == JUR_RET_FAILED) {
          ro->state[q] = JUR_RET_FAILED;
          if (ro->iters[q] == 0) { ro->cost[q] = ro->prior[q] = NAN; ro->nlive[q] = 0; }
        }
      for (long g = 0; g < novj; g++) m->ov_failed += hovp[g];
      for (long g = 0; g < novt; g++) m->ov_cells += hovp[JUR_OVERFLOW_PARTS + g];
    }
    long work = 0;
    for (long r = 0; r < nr_cur; r++) work += reuse ? 1 : rp_cur[r + 1] - rp_cur[r] + 1;
    for (long q = 0; q < nslice; q++) {
      if (ro->state[q] != JUR_RET_ACTIVE) continue;
      ro->cost[q] = hcost[q]; ro->prior[q] = hprior0[q]; ro->nlive[q] = hnlive[q]; ro->iters[q]++;
      J[q] = hcost[q] + hprior0[q];
      for (size_t l = 0; l < RL; l++) Jt[l * RS + (size_t)q] = htcost[l * RS + (size_t)q] + htprior[l * RS + (size_t)q];
    }
    if (ro->h_cost) {
      size_t const at1 = (size_t)it * RS, at2 = (size_t)it * RL * RS;
      for (long q = 0; q < nslice; q++) {
        ro->h_cost[at1 + (size_t)q] = ro->cost[q]; ro->h_prior[at1 + (size_t)q] = ro->prior[q];
        if (ro->state[q] != JUR_RET_ACTIVE) continue;
        for (size_t l = 0; l < RL; l++) {
          size_t const i = l * RS + (size_t)q;
          ro->h_lam[at2 + i] = lamt[i]; ro->h_tcost[at2 + i] = htcost[i]; ro->h_tprior[at2 + i] = htprior[i];
          ro->h_status[at2 + i] = (ovl && hov[RS + i]) ? JUR_TRIAL_OVERFLOW : hstatus[i];
        }
      }
      ro->h_work[2 * it] = work; ro->h_work[2 * it + 1] = nr_cur * rin->nlam;
    }
    if ((rc = jur_retrieve_decide(rin->nlam, nslice, rin->tol, rin->lam_max, fac_max, J, Jt, lamt, hstatus, ro->lam, ro->state, best, accept))) goto done;
    for (long q = 0; q < nslice; q++) {
      choice[q] = accept[q] == 1 ? best[q] : -1;
      if (accept[q] == 1) { ro->cost[q] = htcost[(size_t)best[q] * RS + (size_t)q]; ro->prior[q] = htprior[(size_t)best[q] * RS + (size_t)q]; }
      if (ro->h_best) { ro->h_best[(size_t)it * RS + (size_t)q] = best[q]; ro->h_accept[(size_t)it * RS + (size_t)q] = accept[q]; }
    }
    e = hipMemcpyAsync(d_choice, choice, sizeof(int) * RS, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
    jur_scene_trial_t aq = td.st;
    aq.state = NULL;                                /* (the choice alone says who moves: a slice may just have converged) */
    ek = SCENE_TIMED(m, s, jurk_scene_elements(&aq, JUR_ELEM_ACCEPT, nb, s));
    /* the base segments of the accepted slices are balanced; the others come back with the bits they have */
    if (!ek) ek = scene_hydro_launch(m, s, hy[0], d_base, (size_t)np0);
    if (ek || hipStreamSynchronize(s) != hipSuccess) { (void)hipGetLastError(); jur_set_error("%s: accepting the steps failed", who); rc = JUR_EHIP; goto done; }
  }

  /* what is still active has run out of iterations; the state comes home; the forward model on the retrieved atmosphere,
   * for all rays, from the geometry and the mask that went up at the start */
  if (!(ret = (atm_t *)malloc(sizeof(atm_t)))) { rc = JUR_ENOMEM; goto done; }
  memcpy(ret, atm, sizeof(atm_t));
  if (hyd) {                                      /* the balanced pressures of the base rows; outside the ray slices the caller's */
    e = hipMemcpyAsync(ret->p, d_base + 4 * (size_t)np0, sizeof(double) * (size_t)np0, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipGetLastError(); jur_set_error("%s: bringing the pressures home failed", who); rc = JUR_EHIP; goto done; }
  }
  if (looping) {
    for (long q = 0; q < nslice; q++) if (ro->state[q] == JUR_RET_ACTIVE) ro->state[q] = JUR_RET_MAXITER;
    if (ro->h_cost)
      for (int it = 0; it < rin->max_iter; it++)
        if (ro->h_work[2 * it] == 0)                /* (an iteration that no slice reached) */
          for (long q = 0; q < nslice; q++) { ro->h_cost[(size_t)it * RS + (size_t)q] = ro->cost[q]; ro->h_prior[(size_t)it * RS + (size_t)q] = ro->prior[q]; }
    jur_scene_trial_t xq = td.st;
    xq.out = d_xout;
    int const ek = SCENE_TIMED(m, s, jurk_scene_elements(&xq, JUR_ELEM_STATE, nb, s));
    e = ek ? hipErrorUnknown : hipMemcpyAsync(ro->x, d_xout, sizeof(double) * (size_t)nb, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipGetLastError(); jur_set_error("%s: bringing the state home failed", who); rc = JUR_EHIP; goto done; }
    for (long i = 0; i < nb; i++) scene_row_array(ret, m->view.ng, pl->erow[i])[pl->eip[i]] = ro->x[i];
  }
  if ((rc = jur_model_set_atm(m, ret))) goto done;
  e = hipMemcpyAsync(a->out_rad, d_inrad, sizeof(double) * nrd, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(m->d_status, 0, sizeof(int), s);
  if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
  if ((rc = jur_formod_device(m, nr, d_geom, a->out_rad, a->out_tau, a->out_tp, a->out_np, m->d_status, s))) goto done;
  if (fov) {                                      /* all rays of the call, one slot each */
    fv->k.nr = nr; fv->k.time = d_geom; fv->k.vpz = d_geom + 4 * NR;
    fv->k.r0 = 0; fv->k.r1 = nr; fv->k.ntrial = 1; fv->k.rowptr = NULL;
    fv->k.rad = a->out_rad; fv->k.tau = a->out_tau; fv->k.rad_f = d_frad; fv->k.tau_f = fv->tau;
    if (SCENE_TIMED(m, s, jurk_scene_fov(&fv->k, s))) { rc = launch_failed("%s: field-of-view kernel launch failed", who); goto done; }
    a->out_rad = d_frad; a->out_tau = fv->tau;
  }
  *ret_atm = ret;
  ret = NULL;
done:
  if (rc) (void)hipStreamSynchronize(s);          /* copies out of the arrays freed here may still be under way */
  free(rd); free(ri); free(hact); free(hcomp); free(htimec); free(hjac); free(hov); free(hovp); free(ret);
  return rc;
}

/* nm == NULL: jur_kernel_scene_host.  Otherwise the normal equations of the slices are accumulated on the device after
 * the quotients of every pass, and the blocks go home only where k is given.  With sv (jur_step_scene_host; nm is given
 * then) the systems are solved where they lie after the last pass, and A and b go home only where they are given.  With
 * gd (jur_gradient_scene_host; nm is given then, without A) the passes are forward-only and b, cost and nlive are summed
 * from the caller's blocks.  With pm (jur_param_scene_host) the call is that entry's phase 1 (dg with the gain is given
 * then) or phase 2 (nothing else is given; k may be NULL).  With rt (jur_retrieve_scene_host; nm brings y and weight) the
 * views made here go to retrieve_loop; every other entry has one cut of passes, scene_passes_run's.  who: the entry the
 * messages name.  What the call opens with is scene_open's; of the device slab (scene_slab_reserve) the solver's part is
 * laid out by solve_layout, the diagnostics' by diag_layout and the loop's by loop_layout. */
static int kernel_scene_body(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double *rad, double *tau,
                             double *const tp[3], int *np_out, long const *rowptr, double *k, long max_rays_per_pass,
                             scene_normal_t const *nm, scene_solve_t const *sv, scene_retrieve_t const *rt, scene_diag_t const *dg,
                             scene_grad_t const *gd, scene_param_t *pm, char const *who) {
  { int const ri = scene_ip_check(m, who); if (ri) return ri; }
  if (nr < 0 || max_rays_per_pass < 0) { jur_set_error("%s: bad arguments", who); return JUR_EINVAL; }
  if (sv) { int const rs = solve_check_args(who, sv->in, sv->out); if (rs) return rs; }
  if (rt) m->ov_cells = m->ov_failed = 0;           /* (the counts of jur_model_last_scene_overflow are this call's) */
  if (rt) { int const rs = retrieve_check_args(who, rt->in, rt->out); if (rs) return rs; }
  if (dg) { int const rs = jur_diag_check_out(who, dg->out); if (rs) return rs; }
  int const gn = dg && dg->gin;                     /* jur_gain_scene_host: the blocks are held, the gain follows the diagnostics */
  if (gn) { int const rs = jur_gain_check_args(who, dg->gin, dg->gout); if (rs) return rs; }
  ctl_t const *ctl = m->ctl;
  int rc = scene_atm_check(m, who, "every p, T or H2O element moves every pressure and the Jacobian has no blocks: use jur_kernel", atm);
  if (rc) return rc;
  int const np0 = atm->np, nd = ctl->nd, ng = m->view.ng, nw = m->view.nw;
  if (nr == 0) return JUR_OK;
  if (nr > 0x7fffffffL) { jur_set_error("%s: at most 2^31-1 rays per call", who); return JUR_EINVAL; }
  if (!geom || !rad || !tau || !tp || !rowptr) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }

  size_t const NR = (size_t)nr, nrow = 6 + (size_t)ng + nw;
  int enqueued = 0;
  scene_open_t op;
  long *off = NULL, *pass = NULL, *scopy = NULL, *nptr = NULL;
  int *cdesc = NULL, *iqa = NULL, *ipa = NULL, *srays = NULL;
  int *dmap = NULL, *gmap = NULL;
  long ninv = 0, ndtile = 0, ngtile = 0;
  long *hkoff = NULL;                               /* held blocks: the first double of every ray's | the gradient's workgroups by slice */
  atm_t *ret_atm = NULL;
  int const fov = m->fov_n > 0;                     /* a field of view is set: the radiances of every pass are convolved */
  double const *d_R = NULL;                         /* the model's full prior precision on the device, where one is set */
  int const hyd = m->scene_hydz >= 0;               /* the hydrostatic balance is on: every slice is balanced on its own */
  long *hyat = NULL;                                /* the segment lists of the balance on the host: at | len (ints behind) */
  int const ov = rt && m->scene_overflow == JUR_OVERFLOW_ISOLATE;   /* untraceable rays fail their trial or their slice, not the call */
  trial_plan_t pl;
  memset(&pl, 0, sizeof pl);
  if ((rc = scene_open(&op, m, who, atm, nr, geom, rad, rowptr,
                       (!k && !nm && !pm) ? "%s: null argument" : (gd && !gd->k) ? "%s: null argument (k): the state has elements" : NULL,
                       nm != NULL, nm ? nm->y : NULL, nm ? nm->weight : NULL))) goto done;
  int *const copy0 = op.len + NR, *const sid = op.sid;   /* (copy0: the ints that scene_open leaves to its caller) */
  long const *const rp = op.rp, nslice = op.nslice, nrs = op.nrs;
  jur_scene_slice_t const *const sl = op.sl;
  double const tmax = op.tmax, span = op.span;
  /* the copies of the slices: slice q is raised element by element by the copies scopy[q] ... */
  long ncopies = 0, nt = np0;
  /* what is solved for: the dampings and the prior of the step entry, or of the retrieval's iterations */
  size_t const RS = (size_t)nslice, nlam = sv ? (size_t)sv->in->nlam : rt ? (size_t)rt->in->nlam : 0;
  int const sv_prior = sv ? sv->in->prior_ivar != NULL : rt ? rt->in->prior_ivar != NULL : 0;
  scopy = (long *)malloc(sizeof(long) * ((size_t)nslice + 1));
  if (!scopy) { rc = JUR_ENOMEM; goto done; }
  for (long q = 0; q < nslice; q++) {
    scopy[q] = 1 + ncopies;
    ncopies += sl[q].nel;
    nt += sl[q].nel * sl[q].len;
  }
  for (long r = 0; r < nr; r++)                       /* (a copy beyond 2^31 is refused below with nt) */
    copy0[r] = (sid[r] >= 0 && scopy[sid[r]] <= 0x7fffffffL) ? (int)scopy[sid[r]] : 0;

  /* normal equations: where the sums of every slice lie, its rays as one CSR over the call, its tiles */
  long nlist = 0, ntiles = 0, na = 0, nb = 0;
  long *sptr = NULL, *tptr = NULL, *wptr = NULL, *aptr = NULL;
  if (nm && nslice > 0) {
    if (!rt && ((!sv && !dg && ((!gd && !nm->A) || !nm->b)) || (!dg && (!nm->cost || !nm->nlive)))) { jur_set_error("%s: null argument", who); rc = JUR_EINVAL; goto done; }
    nptr = (long *)calloc(4 * ((size_t)nslice + 1), sizeof(long));
    srays = (int *)malloc(sizeof(int) * NR);
    if (!nptr || !srays) { rc = JUR_ENOMEM; goto done; }
    sptr = nptr; tptr = sptr + nslice + 1; wptr = tptr + nslice + 1; aptr = wptr + nslice + 1;
    nlist = jur_scene_rays_by_slice(nr, nslice, sid, sptr, srays);
    for (long q = 0; q < nslice; q++) {
      long const w = sl[q].nel, T = (w + 15) / 16;
      tptr[q + 1] = tptr[q] + T * (T + 1) / 2;
      wptr[q + 1] = wptr[q] + w;
      aptr[q + 1] = aptr[q] + w * w;
    }
    ntiles = tptr[nslice]; na = aptr[nslice]; nb = wptr[nslice];
    if (gd) na = 0;                                 /* (the gradient has no A: b, cost and nlive alone are accumulated) */
    if (ntiles > 0x7fffffffL) { jur_set_error("%s: 2^31 tiles: call with the rays of fewer slices at a time", who); rc = JUR_EINVAL; goto done; }
    if (sv && (rc = solve_check_values(who, nslice, wptr, sv->in))) goto done;
    if (dg && (rc = jur_diag_check_prior(who, nslice, wptr, dg->prior_ivar))) goto done;
    if (dg && (rc = diag_maps_make(who, nslice, wptr, &ninv, &ndtile, &dmap))) goto done;
    if (gn) {
      /* the variances are read where a measurement can be live: the forward model has not run, F counts as finite */
      if (dg->gin->ncomp > 0) {
        unsigned char *hl = (unsigned char *)malloc(NR * (size_t)nd);
        if (!hl) { rc = JUR_ENOMEM; goto done; }
        double const *const mask = fov ? op.hlive : rad;
        for (size_t at = 0; at < NR * (size_t)nd; at++)
          hl[at] = sid[at / (size_t)nd] >= 0 && isfinite(mask[at]) && isfinite(nm->y[at]) && nm->weight[at] > 0;
        rc = jur_gain_check_var(who, dg->gin->ncomp, nr, nd, dg->gin->var, hl);
        free(hl);
        if (rc) goto done;
      }
      if ((rc = gain_maps_make(who, nslice, wptr, sptr, nd, &ngtile, &gmap))) goto done;
    }
    if (rt) {
      if (rt->in->prior_ivar && (rc = prior_check_values(who, nslice, wptr, rt->in->prior_ivar, rt->in->prior_xa))) goto done;
      /* one atmosphere is the state of all slices only where no point lies in two of them */
      int *owner = (int *)malloc(sizeof(int) * (size_t)np0);
      if (!owner) { rc = JUR_ENOMEM; goto done; }
      for (int i = 0; i < np0; i++) owner[i] = -1;
      for (long q = 0; q < nslice && !rc; q++)
        for (int i = sl[q].first; i < sl[q].first + sl[q].len; i++) {
          if (owner[i] >= 0) {
            jur_set_error("%s: point %d of the atmosphere lies in the slices %d and %ld: their retrievals are not independent", who,
                          i, owner[i], q);
            rc = JUR_EINVAL;
            break;
          }
          owner[i] = (int)q;
        }
      free(owner);
      if (rc) goto done;
      if ((rc = trial_plan_make(&pl, who, m, atm, rt->in->nlam, nr, nslice, sl, sid))) goto done;
    }
  }
  if ((sv || rt || dg) && m->pp_nslice) {           /* a full prior precision is set: of this layout, with prior_ivar */
    long const none[1] = {0};
    if ((rc = prior_precision_for(m, who, nslice, wptr ? wptr : none, dg ? dg->prior_ivar != NULL : sv_prior, &d_R))) goto done;
  }
  /* what the sums add to the slab: the accumulators A | b | cost | nlive, y and weight, the four running sums, the ray lists */
  size_t const nacc = (size_t)na + (size_t)nb + 2 * (size_t)(ntiles ? nslice : 0);
  size_t const acc_bytes = ntiles ? sizeof(double) * (nacc + 2 * NR * (size_t)nd + 4 * ((size_t)nslice + 1)) + sizeof(int) * (size_t)nlist : 0;
  /* ... and the solve: one more copy of the matrices, the vectors of one damping, the outputs of all */
  size_t const nsv = (nlam && ntiles) ? solve_layout((size_t)na, (size_t)nb, RS, nlam, sv_prior, d_R != NULL).end : 0;
  size_t const sv_bytes = sizeof(double) * nsv;
  /* ... or the diagnostics: the factor, S, AVK and the vectors */
  diag_layout_t const dl = diag_layout((size_t)na, (size_t)nb, (size_t)nslice, dg && dg->prior_ivar, d_R != NULL, (size_t)ninv, (size_t)ndtile);
  size_t const ndg = (dg && ntiles) ? dl.end : 0;
  size_t const dg_bytes = sizeof(double) * ndg;
  /* ... and a field of view: the effective mask and the convolved transmittances by ray; for the loop the mask of the
   * rays that remain and the convolved radiances of its last forward model */
  size_t const nfov = fov ? (size_t)(rt ? 4 : 2) * NR * (size_t)nd : 0;
  size_t const fov_bytes = sizeof(double) * nfov;
  long const ncopy = ncopies + 1;
  size_t const atm_bytes = sizeof(double) * (nrow + 1) * (size_t)nt;
  /* ... and the hydrostatic balance: its segment lists (first point and length each) of the base rows' ray slices, of
   * the copies that raise p, T or H2O (at most all) and, in the loop, of the trial copies */
  size_t const NH = hyd ? (size_t)nrs + (size_t)ncopies + (rt ? nlam * RS : 0) : 0;
  size_t const hy_bytes = (sizeof(long) + sizeof(int)) * NH;
  if (nt > 0x7fffffffL || (long)atm_bytes > m->ws_budget / 2) {
    jur_set_error("%s: the stacked atmosphere (%ld points, %zu bytes) exceeds the workspace budget: "
                  "call with the rays of fewer slices at a time", who, nt, atm_bytes);
    rc = JUR_ENOMEM; goto done;
  }
  /* what follows joins the slab part by part, each refused where it no longer fits beside those before it (an entry
   * with diagnostics has no solve, no loop and no held blocks) */
  double used = (double)atm_bytes;
  size_t const side_bytes = pm ? pm->bytes : 0;     /* (what jur_param_scene_host holds beside the slab) */
  if (side_bytes > 0 && !scene_fits(m, &used, side_bytes)) {
    jur_set_error("%s: the gain, the effective weights, C and the parameter covariances (%zu bytes) do not fit beside the stacked "
                  "atmosphere (%zu bytes) in the workspace budget: call with the rays of fewer slices at a time", who, side_bytes, atm_bytes);
    rc = JUR_ENOMEM; goto done;
  }
  if (hy_bytes > 0 && !scene_fits(m, &used, hy_bytes)) {
    jur_set_error("%s: the segment lists of the hydrostatic balance (%zu bytes) do not fit beside the stacked atmosphere (%zu "
                  "bytes) in the workspace budget: call with the rays of fewer slices at a time", who, hy_bytes, atm_bytes);
    rc = JUR_ENOMEM; goto done;
  }
  if (fov_bytes > 0 && !scene_fits(m, &used, fov_bytes)) {
    jur_set_error("%s: the field of view's arrays (%zu bytes) do not fit beside the stacked atmosphere (%zu bytes) "
                  "in the workspace budget: call with fewer rays at a time", who, fov_bytes, atm_bytes);
    rc = JUR_ENOMEM; goto done;
  }
  if (acc_bytes > 0 && !scene_fits(m, &used, acc_bytes)) {
    jur_set_error("%s: the normal matrices (%ld doubles) do not fit beside the stacked atmosphere (%zu bytes) "
                  "in the workspace budget: call with the rays of fewer slices at a time", who, na, atm_bytes + fov_bytes);
    rc = JUR_ENOMEM; goto done;
  }
  if (sv_bytes > 0 && !scene_fits(m, &used, sv_bytes)) {
    jur_set_error("%s: the solver scratch (%zu bytes) does not fit beside the normal matrices (%ld doubles) and the stacked "
                  "atmosphere (%zu bytes) in the workspace budget: call with the rays of fewer slices at a time", who, sv_bytes, na, atm_bytes);
    rc = JUR_ENOMEM; goto done;
  }
  if (dg_bytes > 0 && !scene_fits(m, &used, dg_bytes)) {
    jur_set_error("%s: the factor, S, AVK and the vectors (%zu bytes) do not fit beside the normal matrices (%ld doubles) and the "
                  "stacked atmosphere (%zu bytes) in the workspace budget: call with the rays of fewer slices at a time", who, dg_bytes, na, atm_bytes);
    rc = JUR_ENOMEM; goto done;
  }

  /* ... and the retrieval loop: the trial copies (counted beside the stacked rows, whose memory they share in turn), the
   * trial costs and priors, the prior term and the state, the arrays of the rays that remain once slices have ended
   * (geometry, mask, y, weight; rowptr and sptr of their own), the plan's index arrays: loop_layout */
  int const looping = rt && ntiles;
  size_t const nrd = NR * (size_t)nd;
  loop_layout_t const ll = looping ? loop_layout(&pl, NR, nrd, d_R != NULL, ov) : (loop_layout_t){0, 0, 0, 0, 0, 0, 0};
  size_t const rt_atm_bytes = looping ? sizeof(double) * (nrow + 1) * (size_t)pl.nt : 0;
  size_t const rt_bytes = sizeof(double) * (ll.dbl + ll.lng) + sizeof(int) * ll.ints;
  used += (double)rt_atm_bytes;
  if (looping && !scene_fits(m, &used, rt_bytes)) {
    jur_set_error("%s: the trial copies (%ld points, %zu bytes) and the loop's arrays (%zu bytes) do not fit beside the solver "
                  "scratch, the normal matrices and the stacked atmosphere (%zu bytes) in the workspace budget: call with the rays "
                  "of fewer slices at a time", who, pl.nt, rt_atm_bytes, rt_bytes, atm_bytes + acc_bytes + sv_bytes);
    rc = JUR_ENOMEM; goto done;
  }

  /* ... and the blocks that are held: the caller's (jur_gradient_scene_host), or those a Jacobian iteration of the loop
   * leaves for the reuse iterations (jur_model_set_kernel_recomp).  They take the place of the blocks of a pass; beside
   * them an all-zero rowptr (a forward-only pass has one slot per ray), the first double of every ray's block and the
   * workgroups of the gradient kernel by slice */
  int const every = looping ? m->kernel_recomp : 1;
  int const held = gn && ntiles;                    /* (an entry with the gain has no loop: the blocks of its one Jacobian pass stay) */
  int const retain = gd || every > 1 || held;
  size_t const nkret = retain ? (size_t)rp[nr] * (size_t)nd : 0;
  size_t const nrc = retain ? (NR + 1) + NR + (RS + 1) : 0;
  gain_layout_t const gl = gain_layout(pm ? 0 : nkret, (size_t)nb, nrd, gn ? (size_t)dg->gin->ncomp : 0, (size_t)ngtile);
  size_t const ngn = held ? gl.end : 0;
  size_t const kret_bytes = sizeof(double) * (nkret + nrc + ngn);
  if (held && !scene_fits(m, &used, kret_bytes)) {
    jur_set_error("%s: the retained blocks of all rays (%ld columns, %zu bytes), the gain and the budget's arrays (%zu bytes) do not "
                  "fit beside the stacked atmosphere (%zu bytes), the normal matrices and the diagnostics in the workspace budget: "
                  "call with the rays of fewer slices at a time", who, rp[nr], sizeof(double) * (nkret + nrc), sizeof(double) * ngn, atm_bytes);
    rc = JUR_ENOMEM; goto done;
  }
  if (retain && !held && !scene_fits(m, &used, kret_bytes)) {
    jur_set_error("%s: the blocks of all rays (%ld columns, %zu bytes) do not fit beside the stacked atmosphere (%zu bytes)%s in the "
                  "workspace budget: call with the rays of fewer slices at a time", who, rp[nr], kret_bytes, atm_bytes,
                  gd ? "" : ", the normal matrices and the loop's arrays");
    rc = JUR_ENOMEM; goto done;
  }

  /* passes: contiguous ranges of rays whose slots (width + 1 each) stay within the cap; one ray beyond it goes alone */
  size_t const slot_bytes = sizeof(double) * (10 + (size_t)(fov ? 4 : 3) * (size_t)nd) + sizeof(int);   /* (with the convolved radiances) */
  long cap = max_rays_per_pass;
  /* from the budget, less the parts counted above but for the loop's (the forward model sizes its LOS and transmittance
   * workspace from the budget by itself).  `used` sums byte counts that each fitted into half the budget: exact in double
   * below 2^53, so equal to a sum in long; a budget beyond that gives a cap that is clamped on the next line either way. */
  if (cap == 0) cap = jur_scene_default_cap(m->ws_budget, (long)used - (long)rt_atm_bytes - (long)rt_bytes, slot_bytes);
  if (cap > 0x7fffffffL) cap = 0x7fffffffL;
  long npass = 0, nmax = 0, kmax = 0;
  pass = (long *)malloc(sizeof(long) * 3 * (NR + 1));       /* (second part: the trial passes of the retrieval loop, third: its forward-only passes) */
  if (!pass) { rc = JUR_ENOMEM; goto done; }
  double const *const scan_time = fov ? geom[0] : NULL;
  if (gd) {                                         /* forward-only: one slot per ray, no blocks of a pass */
    if ((npass = jur_trial_passes(nr, 1, cap, scan_time, pass, &nmax)) < 0) { rc = JUR_EINVAL; goto done; }
  } else if ((npass = jur_scene_passes(nr, rp, cap, scan_time, pass, &nmax, &kmax)) < 0) { jur_set_error("%s: a ray with 2^31 state elements", who); rc = JUR_EINVAL; goto done; }
  long *const tpass = pass + NR + 1, *const fpass = tpass + NR + 1;
  long ntpass = 0, nfpass = 0;
  if (looping) {
    if ((ntpass = jur_trial_passes(nr, rt->in->nlam, cap, scan_time, tpass, NULL)) < 0) { jur_set_error("%s: a scan with 2^31 trial rays", who); rc = JUR_EINVAL; goto done; }
    /* once slices have ended the passes of both kinds are cut anew, and a pass of the rays that remain can be larger
     * than any of the first cut: room for every such pass (the arrays of a pass serve both kinds) */
    if ((rc = jur_scene_pass_reserve(nr, rp, cap, rt->in->nlam, scan_time, &nmax, &kmax))) goto done;
    if (nmax > 0x7fffffffL) { jur_set_error("%s: a pass of 2^31 slots", who); rc = JUR_EINVAL; goto done; }
    if (every > 1) {
      /* the forward-only passes of the reuse iterations take one slot per ray where a Jacobian pass takes width + 1 >= 2
       * and a trial pass nlam >= 1: on any subset of the rays they stay within what is reserved.  Not assumed: the first
       * cut is measured here, the re-cuts where they are made. */
      long fmax = 0;
      if ((nfpass = jur_trial_passes(nr, 1, cap, scan_time, fpass, &fmax)) < 0) { rc = JUR_EINVAL; goto done; }
      if (fmax > nmax) { jur_set_error("%s: a forward-only pass of %ld slots, %ld reserved", who, fmax, nmax); rc = JUR_EINVAL; goto done; }
    }
  }
  kmax *= nd;

  /* descriptors of the copies (copy 0: the base) */
  off = (long *)malloc(sizeof(long) * ((size_t)ncopy + 1));
  cdesc = (int *)malloc(sizeof(int) * 3 * (size_t)ncopy);
  iqa = (int *)malloc(sizeof(int) * 2 * (size_t)np0 * (2 + (size_t)ng + nw));
  if (!off || !cdesc || !iqa) { rc = JUR_ENOMEM; goto done; }
  ipa = iqa + (size_t)np0 * (2 + (size_t)ng + nw);
  int *const cfirst = cdesc, *const prow = cdesc + ncopy, *const pip = cdesc + 2 * ncopy;
  off[0] = 0; cfirst[0] = 0; prow[0] = -1; pip[0] = 0;
  off[1] = np0;
  for (long q = 0; q < nslice; q++) {
    long const n = jur_scene_slice_elements(ctl, atm, sl[q].first, sl[q].len, NULL, iqa, ipa);
    if (n != sl[q].nel) { jur_set_error("%s: layout out of step", who); rc = JUR_EINVAL; goto done; }
    for (long e = 0; e < n; e++) {
      long const j = scopy[q] + e;
      cfirst[j] = sl[q].first;
      prow[j] = scene_row_of(iqa[e]);
      pip[j] = ipa[e];
      off[j + 1] = off[j] + sl[q].len;
    }
  }
  /* the balance's segments: the ray slices in the base rows; the copies whose raised row the pressures depend on, in the
   * stacked rows (the others inherit the balanced base: a second balance would return the same bits); every trial copy */
  long nhc = 0, ntc = 0;
  if (hyd && !(hyat = jur_scene_hydro_segments(NH, nr, nrs, op.hyf, ncopy, off, prow, m->view.ig_h2o >= 0 ? 6 + m->view.ig_h2o : -1,
                                               looping ? pl.ncopy : 0, pl.off, &nhc, &ntc))) { rc = JUR_ENOMEM; goto done; }

  /* the device slab: doubles, then 64-bit integers, then 32-bit ones */
  size_t const o_base = 0, o_geom = o_base + nrow * (size_t)np0, o_inrad = o_geom + 7 * NR, o_rad = o_inrad + nrd,
               o_tau = o_rad + nrd, o_tp = o_tau + nrd, o_h = o_tp + 3 * NR, o_k = o_h + (size_t)ncopy,
               o_rowptr = o_k + (retain ? nkret : (size_t)kmax), o_off = o_rowptr + NR + 1, o_y = o_off + (size_t)ncopy + 1;
  /* (the normal equations' part, empty without them: y, weight, the accumulators A | b | cost | nlive in one piece,
   * then sptr | tptr | wptr | aptr, then what the solve needs) */
  size_t const o_w = o_y + (ntiles ? nrd : 0), o_acc = o_w + (ntiles ? nrd : 0), o_nptr = o_acc + nacc,
               o_sv = o_nptr + (ntiles ? 4 * ((size_t)nslice + 1) : 0), o_dg = o_sv + nsv, o_fov = o_dg + ndg, o_rt = o_fov + nfov,
               o_hy = o_rt + ll.dbl + ll.lng, o_rc = o_hy + NH, o_gn = o_rc + nrc, o_int = o_gn + ngn;   /* (o_fov: live | tau by ray, and for the loop live of the remaining rays | rad; o_hy: the balance's first points) */
  size_t const nint0 = 4 * NR + 3 * (size_t)ncopy + (size_t)nlist, nint = nint0 + ll.ints + NH;   /* (the loop's ints follow the others, the balance's lengths those) */
  hipStream_t s;
  if ((rc = scene_slab_reserve(m, who, sizeof(double) * o_int + sizeof(int) * nint, &s))) goto done;
  if ((rc = ensure_io(m, nmax, 0))) goto done;
  if (fov && (rc = scene_fov_reserve(m, (size_t)nmax * (size_t)nd))) goto done;
  {
    double *const D = (double *)m->d_scene;
    long *const L = (long *)m->d_scene;
    int *const I = (int *)(D + o_int);
    int *const d_first = I, *const d_len = I + NR, *const d_copy0 = I + 2 * NR, *const d_np = I + 3 * NR, *const d_cdesc = I + 4 * NR;
    enqueued = 1;
    double *const d_live = D + o_fov;             /* (the effective mask | the convolved transmittances by ray | the loop's) */
    scene_fov_t fv;
    hipError_t e = scene_open_upload(m, s, &op, np0, nr, geom, rad, D + o_base, D + o_geom, D + o_inrad, d_first, 3, d_live, &fv);
    fv.tau = d_live + nrd;
    if (e == hipSuccess) e = hipMemcpyAsync(L + o_rowptr, rp, sizeof(long) * (NR + 1), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(L + o_off, off, sizeof(long) * ((size_t)ncopy + 1), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_cdesc, cdesc, sizeof(int) * 3 * (size_t)ncopy, hipMemcpyHostToDevice, s);
    if (ntiles) {                                 /* the accumulators are zeroed here, once */
      if (e == hipSuccess) e = hipMemcpyAsync(D + o_y, nm->y, sizeof(double) * nrd, hipMemcpyHostToDevice, s);
      if (e == hipSuccess) e = hipMemcpyAsync(D + o_w, nm->weight, sizeof(double) * nrd, hipMemcpyHostToDevice, s);
      if (e == hipSuccess) e = hipMemcpyAsync(L + o_nptr, nptr, sizeof(long) * 4 * ((size_t)nslice + 1), hipMemcpyHostToDevice, s);
      if (e == hipSuccess) e = hipMemcpyAsync(d_cdesc + 3 * ncopy, srays, sizeof(int) * (size_t)nlist, hipMemcpyHostToDevice, s);
      if (e == hipSuccess) e = hipMemsetAsync(D + o_acc, 0, sizeof(double) * nacc, s);
    }
    jur_hyseg_t const hy_all = {(long)NH, L + o_hy, I + nint0 + ll.ints};   /* the ray slices | the raised copies | the trial copies */
    jur_hyseg_t const hy[3] = {jur_hyseg_sub(hy_all, 0, nrs), jur_hyseg_sub(hy_all, nrs, nhc), jur_hyseg_sub(hy_all, nrs + nhc, ntc)};
    if (NH && e == hipSuccess) e = hipMemcpyAsync(L + o_hy, hyat, sizeof(long) * NH, hipMemcpyHostToDevice, s);
    if (NH && e == hipSuccess) e = hipMemcpyAsync(I + nint0 + ll.ints, hyat + NH, sizeof(int) * NH, hipMemcpyHostToDevice, s);
    /* held blocks: the caller's go up as they are laid out, ray r's at rowptr[r] * nd */
    long *const d_zrp = L + o_rc, *const d_koff = d_zrp + NR + 1, *const d_gptr = d_koff + NR;
    long ngroups = 0;
    if (retain) {
      if (!(hkoff = (long *)malloc(sizeof(long) * (NR + RS + 1)))) { rc = JUR_ENOMEM; goto done; }
      long *const hgptr = hkoff + NR;
      hgptr[0] = 0;
      for (long q = 0; q < nslice; q++) hgptr[q + 1] = hgptr[q] + (sl[q].nel + 255) / 256;
      ngroups = ntiles ? hgptr[nslice] : 0;
      if (ngroups > 0x7fffffffL) { jur_set_error("%s: 2^31 workgroups: call with the rays of fewer slices at a time", who); rc = JUR_EINVAL; goto done; }
      for (long r = 0; r < nr; r++) hkoff[r] = rp[r] * nd;
      if (e == hipSuccess) e = hipMemsetAsync(d_zrp, 0, sizeof(long) * (NR + 1), s);
      if (e == hipSuccess) e = hipMemcpyAsync(d_gptr, hgptr, sizeof(long) * (RS + 1), hipMemcpyHostToDevice, s);
      if ((gd || held) && e == hipSuccess) e = hipMemcpyAsync(d_koff, hkoff, sizeof(long) * NR, hipMemcpyHostToDevice, s);
      if (gd && nkret && e == hipSuccess) e = hipMemcpyAsync(D + o_k, gd->k, sizeof(double) * nkret, hipMemcpyHostToDevice, s);
    }
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
    /* the base rows are balanced once, over the ray slices, before the first pass: the caller's atm is never written */
    if (scene_hydro_launch(m, s, hy[0], D + o_base, (size_t)np0)) {
      jur_set_error("%s: hydrostatic kernel launch failed", who); rc = JUR_EHIP; goto done;
    }

    jur_scene_stack_t st;
    memset(&st, 0, sizeof st);
    st.ncopy = (int)ncopy; st.np0 = np0; st.nrow = (int)nrow; st.ng = ng; st.nt = nt;
    st.off = L + o_off; st.first = d_cdesc; st.prow = d_cdesc + ncopy; st.pip = d_cdesc + 2 * ncopy;
    st.base = D + o_base; st.h = D + o_h;
    st.tmax = tmax; st.span = span;
    jur_scene_pass_t a;
    memset(&a, 0, sizeof a);
    a.nr = nr; a.nd = nd;
    a.rowptr = L + o_rowptr; a.first = d_first; a.len = d_len; a.copy0 = d_copy0; a.off = L + o_off;
    a.above = tmax + ((double)ncopy + 1.0) * span;
    a.in_geom = D + o_geom; a.in_rad = D + o_inrad;
    a.h = D + o_h; a.k = D + o_k;
    a.out_rad = D + o_rad; a.out_tau = D + o_tau; a.out_tp = D + o_tp; a.out_np = d_np;
    jur_scene_normal_t nq;
    memset(&nq, 0, sizeof nq);
    if (ntiles) {
      nq.nslice = nslice;
      nq.sptr = L + o_nptr; nq.tptr = nq.sptr + nslice + 1; nq.wptr = nq.tptr + nslice + 1; nq.aptr = nq.wptr + nslice + 1;
      nq.srays = d_cdesc + 3 * ncopy;
      nq.y = D + o_y; nq.weight = D + o_w;
      nq.A = D + o_acc; nq.b = nq.A + na; nq.cost = nq.b + nb; nq.nlive = (long *)(nq.cost + nslice);
    }

    jur_scene_grad_t gq;
    memset(&gq, 0, sizeof gq);
    gq.k = D + o_k; gq.koff = d_koff; gq.gptr = d_gptr;

    if (rt) {
      if ((rc = retrieve_loop(m, s, who, atm, nr, geom[0], rt, &op, &pl, ntiles, na, cap, nmax, pass, npass, ntpass, nfpass, &st, &a, &nq,
                              &gq, &fv, D + o_base, d_zrp, hkoff, hy, d_R, D + o_sv, D + o_rt, I + nint0, d_live + 2 * nrd, &ret_atm))) goto done;
    } else {
      /* the one cut of the call: forward-only for the gradient entry, one slot per ray, which the kernels of a pass make
       * of the all-zero rowptr; with the gain the blocks stay where the pass leaves them */
      scene_cut_t const cut = {pass, npass, rp, gd != NULL, held, D + o_k, k};
      if (gd) a.rowptr = d_zrp;
      if ((rc = scene_passes_run(m, s, who, atm, &st, &a, &nq, ntiles, &gq, ngroups, fov ? &fv : NULL, hy[1], &cut, NULL,
                                 (pm && pm->phase == 2) ? pm : NULL, nmax))) goto done;
      if (nsv && (rc = solve_enqueue(m, s, who, nslice, na, nb, nq.wptr, nq.aptr, nq.A, nq.b, D + o_sv, sv->in, sv->out, NULL, d_R))) goto done;
      if (ndg && (rc = diag_enqueue(m, s, who, nslice, na, nb, nq.wptr, nq.aptr, nq.A, D + o_dg, dg->prior_ivar, dg->out, ninv, ndtile, dmap, d_R))) goto done;
      if (held) {
        /* S and the breakdowns lie where the diagnostics left them, the blocks of all rays where the passes left them; the
         * effective weights are formed from the results of the passes, under the mask the sums were formed under */
        jur_scene_weff_t wq;
        wq.n = (long)nrd; wq.mask = fov ? d_live : D + o_inrad; wq.f = D + o_rad; wq.y = D + o_y; wq.weight = D + o_w;
        wq.weff = D + o_gn + gl.weff;
        if (SCENE_TIMED(m, s, jurk_scene_weff(&wq, s))) { rc = launch_failed("%s: effective-weight kernel launch failed", who); goto done; }
        jur_scene_gain_t gq2;
        memset(&gq2, 0, sizeof gq2);
        gq2.nslice = nslice; gq2.nd = nd; gq2.wptr = nq.wptr; gq2.aptr = nq.aptr; gq2.sptr = nq.sptr; gq2.srays = nq.srays;
        gq2.koff = d_koff; gq2.gptr = d_gptr; gq2.status = (int const *)(D + o_dg + dl.stat); gq2.S = D + o_dg + dl.S; gq2.k = D + o_k;
        gq2.nrd = (long)nrd; gq2.nb = nb;
        if ((rc = gain_enqueue(m, s, who, &gq2, D + o_gn, nkret, ngtile, ngroups, gmap, dg->gin, dg->gout, pm ? pm->gain : NULL))) goto done;
        if (pm && nrd && hipMemcpyAsync(pm->weff, wq.weff, sizeof(double) * nrd, hipMemcpyDeviceToDevice, s) != hipSuccess) {
          (void)hipGetLastError(); jur_set_error("%s: keeping the effective weights failed", who); rc = JUR_EHIP; goto done;
        }
      }
    }
    e = hipMemcpyAsync(rad, a.out_rad, sizeof(double) * nrd, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(tau, a.out_tau, sizeof(double) * nrd, hipMemcpyDeviceToHost, s);
    for (int q = 0; q < 3 && e == hipSuccess; q++) e = hipMemcpyAsync(tp[q], a.out_tp + (size_t)q * NR, sizeof(double) * NR, hipMemcpyDeviceToHost, s);
    if (np_out && e == hipSuccess) e = hipMemcpyAsync(np_out, a.out_np, sizeof(int) * NR, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m->h_status, m->d_status, sizeof(int), hipMemcpyDeviceToHost, s);
    if (ntiles && !rt) {                          /* the sums go home here, once */
      if (nm->A && e == hipSuccess) e = hipMemcpyAsync(nm->A, nq.A, sizeof(double) * (size_t)na, hipMemcpyDeviceToHost, s);
      if (nm->b && e == hipSuccess) e = hipMemcpyAsync(nm->b, nq.b, sizeof(double) * (size_t)nb, hipMemcpyDeviceToHost, s);
      if (nm->cost && e == hipSuccess) e = hipMemcpyAsync(nm->cost, nq.cost, sizeof(double) * (size_t)nslice, hipMemcpyDeviceToHost, s);
      if (nm->nlive && e == hipSuccess) e = hipMemcpyAsync(nm->nlive, nq.nlive, sizeof(long) * (size_t)nslice, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
    rc = scene_status_rc(m, who, ov);
    if (ov && !rc) *m->h_status &= ~1;             /* (the rays that could not be traced are the caller's to read off np_out) */
    if (rt && !rc) memcpy(rt->atm_ret, ret_atm, sizeof(atm_t));
  }
done:
  if (enqueued && rc) (void)hipStreamSynchronize(m->stream);   /* copies out of the arrays freed here may still be under way */
  free(srays); free(scopy); free(nptr); free(off); free(pass); free(cdesc); free(iqa);
  free(ret_atm); free(dmap); free(gmap); free(hyat); free(hkoff);
  scene_open_free(&op);
  trial_plan_free(&pl);
  return rc;
}

/* leave the model with the caller's atmosphere -- after a refusal or an error too: never with the stacked one, which
 * later calls would accept; if it cannot go back, with none ("no atmosphere set") */
static int scene_restore_atm(jur_model_t *m, atm_t const *atm, int rc) {
  if (atm->np < 2 || atm->np > JUR_NP) return rc;
  if ((m->ctl->ip == 2 || m->ctl->ip == 3) && rc != JUR_OK) return rc;   /* scene_ip_check refused the call before the model's atmosphere was touched */
  if (rc == JUR_OK) return jur_model_set_atm(m, atm);
  char msg[512];
  snprintf(msg, sizeof msg, "%s", jur_last_error());
  if (jur_model_set_atm(m, atm) != JUR_OK) { m->view.atm_np = 0; m->h_atm_n = 0; }
  jur_set_error("%s", msg);
  return rc;
}

int jur_kernel_scene_host(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double *rad, double *tau,
                          double *const tp[3], int *np_out, long const *rowptr, double *k, long max_rays_per_pass) {
  if (!m || !atm) { jur_set_error("jur_kernel_scene_host: null argument"); return JUR_EINVAL; }
  return scene_restore_atm(m, atm, kernel_scene_body(m, atm, nr, geom, rad, tau, tp, np_out, rowptr, k, max_rays_per_pass, NULL, NULL, NULL, NULL, NULL, NULL, "jur_kernel_scene_host"));
}

int jur_normal_scene_host(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double *rad, double *tau,
                          double *const tp[3], int *np_out, long const *rowptr, double const *y, double const *weight,
                          double *A, double *b, double *cost, long *nlive, double *k, long max_rays_per_pass) {
  if (!m || !atm) { jur_set_error("jur_normal_scene_host: null argument"); return JUR_EINVAL; }
  scene_normal_t const nm = {y, weight, A, b, cost, nlive};
  return scene_restore_atm(m, atm, kernel_scene_body(m, atm, nr, geom, rad, tau, tp, np_out, rowptr, k, max_rays_per_pass, &nm, NULL, NULL, NULL, NULL, NULL, "jur_normal_scene_host"));
}

int jur_gradient_scene_host(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double *rad, double *tau,
                            double *const tp[3], int *np_out, long const *rowptr, double const *y, double const *weight,
                            double const *k, double *b, double *cost, long *nlive, long max_rays_per_pass) {
  if (!m || !atm) { jur_set_error("jur_gradient_scene_host: null argument"); return JUR_EINVAL; }
  scene_normal_t const nm = {y, weight, NULL, b, cost, nlive};
  scene_grad_t const gd = {k};
  return scene_restore_atm(m, atm, kernel_scene_body(m, atm, nr, geom, rad, tau, tp, np_out, rowptr, NULL, max_rays_per_pass, &nm, NULL, NULL, NULL, &gd, NULL, "jur_gradient_scene_host"));
}

int jur_step_scene_host(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double *rad, double *tau,
                        double *const tp[3], int *np_out, long const *rowptr, double const *y, double const *weight,
                        jur_solve_in_t const *in, jur_solve_out_t const *out,
                        double *A, double *b, double *cost, long *nlive, double *k, long max_rays_per_pass) {
  if (!m || !atm) { jur_set_error("jur_step_scene_host: null argument"); return JUR_EINVAL; }
  scene_normal_t const nm = {y, weight, A, b, cost, nlive};
  scene_solve_t const sv = {in, out};
  return scene_restore_atm(m, atm, kernel_scene_body(m, atm, nr, geom, rad, tau, tp, np_out, rowptr, k, max_rays_per_pass, &nm, &sv, NULL, NULL, NULL, NULL, "jur_step_scene_host"));
}

int jur_diagnose_scene_host(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double *rad, double *tau,
                            double *const tp[3], int *np_out, long const *rowptr, double const *y, double const *weight,
                            double const *prior_ivar, jur_diag_out_t const *out,
                            double *A, double *b, double *cost, long *nlive, double *k, long max_rays_per_pass) {
  if (!m || !atm) { jur_set_error("jur_diagnose_scene_host: null argument"); return JUR_EINVAL; }
  scene_normal_t const nm = {y, weight, A, b, cost, nlive};
  scene_diag_t const dg = {prior_ivar, out, NULL, NULL};
  return scene_restore_atm(m, atm, kernel_scene_body(m, atm, nr, geom, rad, tau, tp, np_out, rowptr, k, max_rays_per_pass, &nm, NULL, NULL, &dg, NULL, NULL, "jur_diagnose_scene_host"));
}

int jur_gain_scene_host(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double *rad, double *tau,
                        double *const tp[3], int *np_out, long const *rowptr, double const *y, double const *weight,
                        double const *prior_ivar, jur_diag_out_t const *diag, jur_gain_in_t const *in, jur_gain_out_t const *out,
                        double *A, double *b, double *cost, long *nlive, double *k, long max_rays_per_pass) {
  if (!m || !atm || !in || !out) { jur_set_error("jur_gain_scene_host: null argument"); return JUR_EINVAL; }
  scene_normal_t const nm = {y, weight, A, b, cost, nlive};
  scene_diag_t const dg = {prior_ivar, diag, in, out};
  return scene_restore_atm(m, atm, kernel_scene_body(m, atm, nr, geom, rad, tau, tp, np_out, rowptr, k, max_rays_per_pass, &nm, NULL, NULL, &dg, NULL, NULL, "jur_gain_scene_host"));
}

int jur_retrieve_scene_host(jur_model_t *m, atm_t const *atm0, atm_t *atm_ret, long nr, double const *const geom[7],
                            double *rad, double *tau, double *const tp[3], int *np_out, long const *rowptr,
                            double const *y, double const *weight, jur_retrieve_in_t const *in,
                            jur_retrieve_out_t const *out, long max_rays_per_pass) {
  if (!m || !atm0 || !atm_ret) { jur_set_error("jur_retrieve_scene_host: null argument"); return JUR_EINVAL; }
  scene_normal_t const nm = {y, weight, NULL, NULL, NULL, NULL};
  scene_retrieve_t const rt = {in, out, atm_ret};
  int const rc = kernel_scene_body(m, atm0, nr, geom, rad, tau, tp, np_out, rowptr, NULL, max_rays_per_pass, &nm, NULL, &rt, NULL, NULL, NULL, "jur_retrieve_scene_host");
  if (rc) return scene_restore_atm(m, atm0, rc);    /* (on success the model holds atm_ret) */
  if (nr != 0) return JUR_OK;
  if (atm_ret != atm0) memcpy(atm_ret, atm0, sizeof(atm_t));   /* no rays: nothing was retrieved */
  return scene_restore_atm(m, atm0, JUR_OK);
}

/* The device slab of the scene entries serves: doubles (base rows, geometry, mask, y, weight, dx, the prior pair, cost,
 * prior), then the plan's longs, then its ints. */
static int trial_scene_body(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double const *rad_in,
                            long const *rowptr, double const *y, double const *weight, int ntrial, double const *dx,
                            double const *prior_ivar, double const *prior_xa, double *cost, double *prior, long max_rays_per_pass) {
  char const *const who = "jur_trial_scene_host";
  { int const ri = scene_ip_check(m, who); if (ri) return ri; }
  m->ov_cells = m->ov_failed = 0;                   /* (the counts of jur_model_last_scene_overflow are this call's) */
  if (nr < 0 || max_rays_per_pass < 0) { jur_set_error("%s: bad arguments", who); return JUR_EINVAL; }
  if (ntrial < 1 || ntrial > 64) { jur_set_error("%s: ntrial = %d: 1 to 64 trials per call", who, ntrial); return JUR_EINVAL; }
  if (!prior_ivar != !prior_xa) {
    jur_set_error("%s: %s without %s: the prior is given as a pair", who, prior_ivar ? "prior_ivar" : "prior_xa",
                  prior_ivar ? "prior_xa" : "prior_ivar");
    return JUR_EINVAL;
  }
  ctl_t const *ctl = m->ctl;
  int rc = scene_atm_check(m, who, "a step of one slice moves every pressure: the slices are no independent problems", atm);
  if (rc) return rc;
  int const np0 = atm->np, nd = ctl->nd, ng = m->view.ng, nw = m->view.nw;
  if (nr == 0) return JUR_OK;
  if (nr > 0x7fffffffL / ntrial) { jur_set_error("%s: at most 2^31-1 trial rays per call", who); return JUR_EINVAL; }
  if (!geom || !rad_in || !rowptr || !y || !weight) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }

  size_t const NR = (size_t)nr, nrow = 6 + (size_t)ng + nw, nrd = NR * (size_t)nd;
  int enqueued = 0;
  scene_open_t op;
  long *pass = NULL;
  int const fov = m->fov_n > 0;                     /* a field of view is set: the trial radiances are convolved */
  int const hyd = m->scene_hydz >= 0;               /* the hydrostatic balance is on: base rows and trial copies are balanced */
  long *hyat = NULL;
  int const ov = m->scene_overflow == JUR_OVERFLOW_ISOLATE;   /* an untraceable ray makes its trial's cost NaN, not the call fail */
  trial_plan_t pl;
  memset(&pl, 0, sizeof pl);
  if ((rc = scene_open(&op, m, who, atm, nr, geom, rad_in, rowptr, NULL, 1, y, weight))) goto done;
  long const nslice = op.nslice, nrs = op.nrs;
  if (nslice == 0) goto done;                         /* no state elements: nothing to write */
  if (!dx || !cost || !prior) { jur_set_error("%s: null argument", who); rc = JUR_EINVAL; goto done; }
  if ((rc = trial_plan_make(&pl, who, m, atm, ntrial, nr, nslice, op.sl, op.sid))) goto done;
  long const nb = pl.nb;
  for (int t = 0; t < ntrial; t++)
    for (long q = 0; q < nslice; q++)
      for (long e = pl.wptr[q]; e < pl.wptr[q + 1]; e++)
        if (!isfinite(dx[(size_t)t * (size_t)nb + (size_t)e])) {
          jur_set_error("%s: dx of trial %d, slice %ld, element %ld is %g: not finite", who, t, q, e - pl.wptr[q],
                        dx[(size_t)t * (size_t)nb + (size_t)e]);
          rc = JUR_EINVAL;
          goto done;
        }
  if (prior_ivar && (rc = prior_check_values(who, nslice, pl.wptr, prior_ivar, prior_xa))) goto done;
  double const *d_R = NULL;
  if ((rc = prior_precision_for(m, who, nslice, pl.wptr, prior_ivar != NULL, &d_R))) goto done;

  size_t const NB = (size_t)nb, NS = (size_t)nslice, NT = (size_t)ntrial, npr = prior_ivar ? NB : 0;
  size_t const ndv = d_R ? NT * NB : 0;               /* (a full prior precision: xa - (x + dx) of every trial) */
  size_t const nbd = pl.box ? 2 * NB : 0;             /* (a box on the state: lo | hi of every element) */
  size_t const atm_bytes = sizeof(double) * (nrow + 1) * (size_t)pl.nt;
  size_t const nfov = fov ? nrd : 0;                  /* (the effective mask) */
  size_t const NH = hyd ? (size_t)nrs + NT * NS : 0;  /* (the balance's segments: the ray slices, every trial copy) */
  size_t const nov_int = ov ? NT * NS : 0, nov_lng = ov ? (size_t)JUR_OVERFLOW_PARTS : 0;   /* (the trials' flags, the fold's partial counts) */
  size_t const acc_bytes = sizeof(double) * (NT * NB + 2 * npr + 2 * NT * NS + nfov + ndv + nbd) + (sizeof(long) + sizeof(int)) * NH +
                           sizeof(long) * nov_lng + sizeof(int) * nov_int;
  if ((double)atm_bytes + (double)acc_bytes > (double)(m->ws_budget / 2)) {
    jur_set_error("%s: the trial copies (%ld points, %zu bytes) and accumulators (%zu bytes) exceed the workspace budget: "
                  "call with fewer trials or the rays of fewer slices at a time", who, pl.nt, atm_bytes, acc_bytes);
    rc = JUR_ENOMEM;
    goto done;
  }
  size_t const slot_bytes = sizeof(double) * (10 + (size_t)(fov ? 4 : 3) * (size_t)nd) + sizeof(int);
  long cap = max_rays_per_pass;
  if (cap == 0) cap = jur_scene_default_cap(m->ws_budget, (long)atm_bytes + (long)acc_bytes, slot_bytes);   /* as the Jacobian entries size their passes */
  long nmax = 0;
  if (!(pass = (long *)malloc(sizeof(long) * (NR + 1)))) { rc = JUR_ENOMEM; goto done; }
  long const npass = jur_trial_passes(nr, ntrial, cap, fov ? geom[0] : NULL, pass, &nmax);
  if (npass < 0) { jur_set_error("%s: a scan with 2^31 trial rays", who); rc = JUR_EINVAL; goto done; }

  long nhc = 0, ntc = 0;                              /* (the balance's segments: no raised copies here, every trial copy) */
  if (hyd && !(hyat = jur_scene_hydro_segments(NH, nr, nrs, op.hyf, 0, NULL, NULL, -1, pl.ncopy, pl.off, &nhc, &ntc))) { rc = JUR_ENOMEM; goto done; }

  size_t const o_base = 0, o_geom = o_base + nrow * (size_t)np0, o_inrad = o_geom + 7 * NR, o_y = o_inrad + nrd, o_w = o_y + nrd,
               o_dx = o_w + nrd, o_r = o_dx + NT * NB, o_xa = o_r + npr, o_cost = o_xa + npr, o_prior = o_cost + NT * NS,
               o_live = o_prior + NT * NS, o_dv = o_live + nfov, o_bd = o_dv + ndv, o_long = o_bd + nbd,
               o_int = o_long + pl.nlong + NH + nov_lng;   /* (the balance's first points behind the plan's longs, its lengths behind the ints; the fold's counts and the flags behind those) */
  hipStream_t s;
  if ((rc = scene_slab_reserve(m, who, sizeof(double) * o_int + sizeof(int) * (pl.nint + 2 * NR + NH + nov_int), &s))) goto done;
  if ((rc = ensure_io(m, nmax, 0))) goto done;
  if (fov && (rc = scene_fov_reserve(m, (size_t)nmax * (size_t)nd))) goto done;
  {
    double *const D = (double *)m->d_scene;
    long *const L = (long *)(D + o_long);
    int *const I = (int *)(D + o_int), *const d_first = I + pl.nint, *const d_len = d_first + NR;
    enqueued = 1;
    scene_fov_t fv;
    hipError_t e = scene_open_upload(m, s, &op, np0, nr, geom, rad_in, D + o_base, D + o_geom, D + o_inrad, d_first, 2, D + o_live, &fv);
    if (e == hipSuccess) e = hipMemcpyAsync(D + o_y, y, sizeof(double) * nrd, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(D + o_w, weight, sizeof(double) * nrd, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && NB) e = hipMemcpyAsync(D + o_dx, dx, sizeof(double) * NT * NB, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && npr) e = hipMemcpyAsync(D + o_r, prior_ivar, sizeof(double) * NB, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && npr) e = hipMemcpyAsync(D + o_xa, prior_xa, sizeof(double) * NB, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(L, pl.longs, sizeof(long) * pl.nlong, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(I, pl.ints, sizeof(int) * pl.nint, hipMemcpyHostToDevice, s);
    if (nbd && e == hipSuccess) e = hipMemcpyAsync(D + o_bd, pl.box, sizeof(double) * nbd, hipMemcpyHostToDevice, s);
    jur_hyseg_t const hy = {(long)NH, L + pl.nlong, d_len + NR};
    if (NH && e == hipSuccess) e = hipMemcpyAsync(L + pl.nlong, hyat, sizeof(long) * NH, hipMemcpyHostToDevice, s);
    if (NH && e == hipSuccess) e = hipMemcpyAsync(d_len + NR, hyat + NH, sizeof(int) * NH, hipMemcpyHostToDevice, s);
    long *const d_ovp = L + pl.nlong + NH;
    int *const d_otflag = d_len + NR + NH;
    if (ov && e == hipSuccess) e = hipMemsetAsync(d_otflag, 0, sizeof(int) * nov_int, s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
    if (scene_hydro_launch(m, s, jur_hyseg_sub(hy, 0, nrs), D + o_base, (size_t)np0)) {   /* the base rows, once */
      jur_set_error("%s: hydrostatic kernel launch failed", who); rc = JUR_EHIP; goto done;
    }

    trial_dev_t td;                                 /* (the running sums of w^2 under a full prior precision are the model's own) */
    trial_dev_fill(&td, m, &pl, np0, op.tmax, op.span, L, I, D + o_base, D + o_geom, D + o_inrad, d_first, d_len, D + o_y, D + o_w,
                   D + o_dx, npr ? D + o_r : NULL, npr ? D + o_xa : NULL, D + o_prior, D + o_cost, nbd ? D + o_bd : NULL, d_R,
                   d_R ? (long const *)m->d_pp + NS + 1 : NULL, D + o_dv, ov ? d_otflag : NULL, d_ovp, NULL, NULL);
    long const novt = jur_scene_overflow_parts((long)(NT * NS));
    long hovp[JUR_OVERFLOW_PARTS];
    if ((rc = trial_run(m, s, who, atm, &td, nb, npass, pass, nmax, fov ? &fv : NULL, jur_hyseg_sub(hy, nrs + nhc, ntc)))) goto done;
    e = hipMemcpyAsync(cost, D + o_cost, sizeof(double) * NT * NS, hipMemcpyDeviceToHost, s);
    if (ov && e == hipSuccess) e = hipMemcpyAsync(hovp, d_ovp, sizeof(long) * (size_t)novt, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(prior, D + o_prior, sizeof(double) * NT * NS, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m->h_status, m->d_status, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
    rc = scene_status_rc(m, who, ov);
    if (ov && !rc) {
      *m->h_status &= ~1;
      for (long g = 0; g < novt; g++) m->ov_cells += hovp[g];
    }
  }
done:
  if (enqueued && rc) (void)hipStreamSynchronize(m->stream);
  free(pass); free(hyat);
  scene_open_free(&op);
  trial_plan_free(&pl);
  return rc;
}

int jur_trial_scene_host(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double const *rad_in,
                         long const *rowptr, double const *y, double const *weight, int ntrial, double const *dx,
                         double const *prior_ivar, double const *prior_xa, double *cost, double *prior, long max_rays_per_pass) {
  if (!m || !atm) { jur_set_error("jur_trial_scene_host: null argument"); return JUR_EINVAL; }
  return scene_restore_atm(m, atm, trial_scene_body(m, atm, nr, geom, rad_in, rowptr, y, weight, ntrial, dx, prior_ivar, prior_xa,
                                                    cost, prior, max_rays_per_pass));
}

/* The balance alone, on an atmosphere the caller holds.  The device slab of the scene entries serves (it holds nothing
 * between calls): the rows z | lat | p | T | q_H2O, then the segments' first points and lengths.  Neither the model's
 * atmosphere nor the forward model's workspace is touched. */
int jur_scene_hydrostatic_host(jur_model_t *m, atm_t const *atm_in, long nr, double const *time, atm_t *atm_out) {
  char const *const who = "jur_scene_hydrostatic_host";
  if (!m || !atm_in || !atm_out || nr < 0 || (nr > 0 && !time)) { jur_set_error("%s: bad arguments", who); return JUR_EINVAL; }
  if (!(m->scene_hydz >= 0)) { jur_set_error("%s: the hydrostatic balance of the model is switched off (jur_model_set_scene_hydz)", who); return JUR_EINVAL; }
  int const np = atm_in->np;
  if (np < 2 || np > JUR_NP) { jur_set_error("%s: need 2..%d atmospheric points", who, JUR_NP); return JUR_EINVAL; }
  size_t const NR = (size_t)(nr > 0 ? nr : 1), N = (size_t)np;
  int rc = JUR_OK, enqueued = 0;
  int *first = (int *)malloc(sizeof(int) * 4 * NR), *len = first ? first + NR : NULL, *sf = first ? len + NR : NULL, *sn = first ? sf + NR : NULL;
  long *at = NULL;
  double *h = NULL;
  if (!first) { jur_set_error("%s: out of memory", who); return JUR_ENOMEM; }
  for (long r = 0; r < nr; r++) {
    long lo;
    len[r] = jur_atm_slice(atm_in->time, np, time[r], &lo);
    first[r] = (int)lo;
  }
  long const nseg = jur_scene_ray_slices_of(np, nr, first, len, sf, sn);
  if (nseg < 0) { jur_set_error("%s: out of memory", who); rc = JUR_ENOMEM; goto done; }
  if ((rc = jur_scene_hydro_check(who, np, nseg, sf, sn))) goto done;
  {
    int const ig = m->view.ig_h2o;
    size_t const NS = (size_t)nseg, o_at = 5 * N, o_len = o_at + NS;
    size_t const bytes = sizeof(double) * o_len + sizeof(int) * (NS + 1);
    at = (long *)malloc(sizeof(long) * (NS + 1));
    h = (double *)malloc(sizeof(double) * 5 * N);
    if (!at || !h) { jur_set_error("%s: out of memory", who); rc = JUR_ENOMEM; goto done; }
    for (long q = 0; q < nseg; q++) at[q] = sf[q];
    memcpy(h, atm_in->z, sizeof(double) * N);
    memcpy(h + N, atm_in->lat, sizeof(double) * N);
    memcpy(h + 2 * N, atm_in->p, sizeof(double) * N);
    memcpy(h + 3 * N, atm_in->t, sizeof(double) * N);
    if (ig >= 0) memcpy(h + 4 * N, atm_in->q[ig], sizeof(double) * N);
    hipStream_t s;
    if ((rc = scene_slab_reserve(m, who, bytes, &s))) goto done;
    double *const D = (double *)m->d_scene;
    long *const d_at = (long *)(D + o_at);
    int *const d_len = (int *)(D + o_len);
    enqueued = 1;
    hipError_t e = hipMemcpyAsync(D, h, sizeof(double) * (ig >= 0 ? 5 : 4) * N, hipMemcpyHostToDevice, s);
    if (nseg && e == hipSuccess) e = hipMemcpyAsync(d_at, at, sizeof(long) * NS, hipMemcpyHostToDevice, s);
    if (nseg && e == hipSuccess) e = hipMemcpyAsync(d_len, sn, sizeof(int) * NS, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
    jur_scene_hydro_t hq;
    memset(&hq, 0, sizeof hq);
    hq.nseg = nseg; hq.at = d_at; hq.len = d_len; hq.hydz = m->scene_hydz;
    hq.z = D; hq.lat = D + N; hq.p = D + 2 * N; hq.t = D + 3 * N; hq.q = ig >= 0 ? D + 4 * N : NULL;
    if (SCENE_TIMED(m, s, jurk_scene_hydro(&hq, s))) { rc = launch_failed("%s: hydrostatic kernel launch failed", who); goto done; }
    e = hipMemcpyAsync(h + 2 * N, D + 2 * N, sizeof(double) * N, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
    if (atm_out != atm_in) memcpy(atm_out, atm_in, sizeof(atm_t));
    memcpy(atm_out->p, h + 2 * N, sizeof(double) * N);
  }
done:
  if (enqueued && rc) (void)hipStreamSynchronize(m->stream);
  free(first); free(at); free(h);
  return rc;
}

/* Systems the caller holds.  The device slab of the scene entries serves (it holds nothing between calls): wptr | aptr,
 * A, b, then the solver's part.  Neither the atmosphere nor the forward model's workspace is touched. */
int jur_solve_slices_host(jur_model_t *m, long nslice, long const *wptr, double const *A, double const *b,
                          jur_solve_in_t const *in, jur_solve_out_t const *out) {
  char const *const who = "jur_solve_slices_host";
  if (!m || nslice < 0) { jur_set_error("%s: bad arguments", who); return JUR_EINVAL; }
  int rc = solve_check_args(who, in, out);
  if (rc) return rc;
  if (nslice == 0) return JUR_OK;
  if (nslice > 0x7fffffffL) { jur_set_error("%s: at most 2^31-1 systems per call", who); return JUR_EINVAL; }
  if (!wptr || !A || !b) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  size_t const NS = (size_t)nslice;
  long *ptr = (long *)malloc(sizeof(long) * 2 * (NS + 1)), *aptr = ptr ? ptr + NS + 1 : NULL;
  if (!ptr) return JUR_ENOMEM;
  int enqueued = 0;
  aptr[0] = 0;
  for (long q = 0; q < nslice; q++) {
    long const w = wptr[q + 1] - wptr[q];
    if (wptr[0] != 0 || w < 0 || w > 0x7fffffffL) {
      jur_set_error("%s: wptr is not an ascending running sum of widths from 0 (slice %ld)", who, q);
      rc = JUR_EINVAL;
      goto done;
    }
    aptr[q + 1] = aptr[q] + w * w;
  }
  memcpy(ptr, wptr, sizeof(long) * (NS + 1));
  if ((rc = solve_check_values(who, nslice, wptr, in))) goto done;
  double const *d_R = NULL;
  if ((rc = prior_precision_for(m, who, nslice, wptr, in->prior_ivar != NULL, &d_R))) goto done;
  {
    long const na = aptr[nslice], nb = wptr[nslice];
    size_t const o_A = 2 * (NS + 1), o_b = o_A + (size_t)na, o_sv = o_b + (size_t)nb;
    size_t const nsv = solve_layout((size_t)na, (size_t)nb, NS, (size_t)in->nlam, in->prior_ivar != NULL, d_R != NULL).end;
    hipStream_t s;
    if ((rc = scene_slab_reserve(m, who, sizeof(double) * (o_sv + nsv), &s))) goto done;
    double *const D = (double *)m->d_scene;
    long *const L = (long *)m->d_scene;
    enqueued = 1;
    hipError_t e = hipMemcpyAsync(L, ptr, sizeof(long) * 2 * (NS + 1), hipMemcpyHostToDevice, s);
    if (na && e == hipSuccess) e = hipMemcpyAsync(D + o_A, A, sizeof(double) * (size_t)na, hipMemcpyHostToDevice, s);
    if (nb && e == hipSuccess) e = hipMemcpyAsync(D + o_b, b, sizeof(double) * (size_t)nb, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
    if ((rc = solve_enqueue(m, s, who, nslice, na, nb, L, L + NS + 1, D + o_A, D + o_b, D + o_sv, in, out, NULL, d_R))) goto done;
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; }
  }
done:
  if (enqueued && rc) (void)hipStreamSynchronize(m->stream);
  free(ptr);
  return rc;
}

/* Systems the caller holds, as jur_solve_slices_host: wptr | aptr, A, then the diagnostics' part of the slab. */
int jur_diagnose_slices_host(jur_model_t *m, long nslice, long const *wptr, double const *A, double const *prior_ivar,
                             jur_diag_out_t const *out) {
  char const *const who = "jur_diagnose_slices_host";
  if (!m || nslice < 0) { jur_set_error("%s: bad arguments", who); return JUR_EINVAL; }
  int rc = jur_diag_check_out(who, out);
  if (rc) return rc;
  if (nslice == 0) return JUR_OK;
  if (nslice > 0x7fffffffL) { jur_set_error("%s: at most 2^31-1 systems per call", who); return JUR_EINVAL; }
  if (!wptr) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  if ((rc = jur_diag_check_wptr(who, nslice, wptr))) return rc;
  if (wptr[nslice] > 0 && !A) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  if ((rc = jur_diag_check_prior(who, nslice, wptr, prior_ivar))) return rc;
  size_t const NS = (size_t)nslice;
  long *ptr = (long *)malloc(sizeof(long) * 2 * (NS + 1)), *aptr = ptr ? ptr + NS + 1 : NULL;
  int *hmap = NULL;
  long ninv = 0, ntile = 0;
  if (!ptr) return JUR_ENOMEM;
  int enqueued = 0;
  memcpy(ptr, wptr, sizeof(long) * (NS + 1));
  aptr[0] = 0;
  for (long q = 0; q < nslice; q++) { long const w = wptr[q + 1] - wptr[q]; aptr[q + 1] = aptr[q] + w * w; }
  if ((rc = diag_maps_make(who, nslice, wptr, &ninv, &ntile, &hmap))) goto done;
  double const *d_R = NULL;
  if ((rc = prior_precision_for(m, who, nslice, wptr, prior_ivar != NULL, &d_R))) goto done;
  {
    long const na = aptr[nslice], nb = wptr[nslice];
    size_t const o_A = 2 * (NS + 1), o_dg = o_A + (size_t)na;
    size_t const ndg = diag_layout((size_t)na, (size_t)nb, NS, prior_ivar != NULL, d_R != NULL, (size_t)ninv, (size_t)ntile).end;
    hipStream_t s;
    if ((rc = scene_slab_reserve(m, who, sizeof(double) * (o_dg + ndg), &s))) goto done;
    double *const D = (double *)m->d_scene;
    long *const L = (long *)m->d_scene;
    enqueued = 1;
    hipError_t e = hipMemcpyAsync(L, ptr, sizeof(long) * 2 * (NS + 1), hipMemcpyHostToDevice, s);
    if (na && e == hipSuccess) e = hipMemcpyAsync(D + o_A, A, sizeof(double) * (size_t)na, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
    if ((rc = diag_enqueue(m, s, who, nslice, na, nb, L, L + NS + 1, D + o_A, D + o_dg, prior_ivar, out, ninv, ntile, hmap, d_R))) goto done;
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; }
  }
done:
  if (enqueued && rc) (void)hipStreamSynchronize(m->stream);
  free(ptr); free(hmap);
  return rc;
}

/* Systems and blocks the caller holds: wptr | aptr | sptr | gptr | koff, S, k, then the gain's part of the slab, then the
 * ints status | srays. */
int jur_gain_slices_host(jur_model_t *m, long nslice, long const *wptr, double const *S, int const *status, long nr, int nd,
                         long const *rowptr, int const *sid, double const *k, double const *weight_eff,
                         jur_gain_in_t const *in, jur_gain_out_t const *out) {
  char const *const who = "jur_gain_slices_host";
  if (!m || nslice < 0 || nr < 0 || nd < 0) { jur_set_error("%s: bad arguments", who); return JUR_EINVAL; }
  int rc = jur_gain_check_args(who, in, out);
  if (rc) return rc;
  if (nslice == 0 || nr == 0) return JUR_OK;
  if (nslice > 0x7fffffffL || nr > 0x7fffffffL) { jur_set_error("%s: at most 2^31-1 systems and rays per call", who); return JUR_EINVAL; }
  if (!wptr || !rowptr || !sid) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  if ((rc = jur_diag_check_wptr(who, nslice, wptr))) return rc;
  if ((rc = jur_gain_check_layout(who, nslice, wptr, nr, rowptr, sid))) return rc;
  size_t const NS = (size_t)nslice, NR = (size_t)nr, nrd = NR * (size_t)nd, nk = (size_t)rowptr[nr] * (size_t)nd;
  if ((wptr[nslice] > 0 && !S) || (nk > 0 && !k) || (nrd > 0 && !weight_eff)) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  long *ptr = (long *)malloc(sizeof(long) * (4 * (NS + 1) + NR));
  int *srays = (int *)malloc(sizeof(int) * NR), *hmap = NULL;
  unsigned char *hl = (unsigned char *)malloc(nrd ? nrd : 1);
  int enqueued = 0;
  if (!ptr || !srays || !hl) { jur_set_error("%s: out of memory", who); rc = JUR_ENOMEM; goto done; }
  {
    long *const aptr = ptr + NS + 1, *const sptr = aptr + NS + 1, *const gptr = sptr + NS + 1, *const koff = gptr + NS + 1;
    long ntile = 0;
    memcpy(ptr, wptr, sizeof(long) * (NS + 1));
    aptr[0] = 0; gptr[0] = 0;
    for (long q = 0; q < nslice; q++) {
      long const w = wptr[q + 1] - wptr[q];
      aptr[q + 1] = aptr[q] + w * w;
      gptr[q + 1] = gptr[q] + (w + 255) / 256;
    }
    for (long r = 0; r < nr; r++) koff[r] = rowptr[r] * nd;
    long const nlist = jur_scene_rays_by_slice(nr, nslice, sid, sptr, srays);
    for (size_t at = 0; at < nrd; at++) hl[at] = sid[at / (size_t)nd] >= 0 && weight_eff[at] > 0;
    if (in->ncomp > 0 && (rc = jur_gain_check_var(who, in->ncomp, nr, nd, in->var, hl))) goto done;
    if ((rc = gain_maps_make(who, nslice, wptr, sptr, nd, &ntile, &hmap))) goto done;
    long const na = aptr[nslice], nb = wptr[nslice], ngroups = gptr[nslice];
    if (ngroups > 0x7fffffffL) { jur_set_error("%s: 2^31 workgroups: call with fewer systems at a time", who); rc = JUR_EINVAL; goto done; }
    size_t const nlong = 4 * (NS + 1) + NR, o_S = nlong, o_k = o_S + (size_t)na, o_gn = o_k + nk;
    gain_layout_t const gl = gain_layout(nk, (size_t)nb, nrd, (size_t)in->ncomp, (size_t)ntile);
    size_t const o_int = o_gn + gl.end;
    hipStream_t s;
    if ((rc = scene_slab_reserve(m, who, sizeof(double) * o_int + sizeof(int) * (NS + (size_t)nlist + 1), &s))) goto done;
    double *const D = (double *)m->d_scene;
    long *const L = (long *)m->d_scene;
    int *const d_stat = (int *)(D + o_int), *const d_srays = d_stat + NS;
    enqueued = 1;
    hipError_t e = hipMemcpyAsync(L, ptr, sizeof(long) * nlong, hipMemcpyHostToDevice, s);
    if (na && e == hipSuccess) e = hipMemcpyAsync(D + o_S, S, sizeof(double) * (size_t)na, hipMemcpyHostToDevice, s);
    if (nk && e == hipSuccess) e = hipMemcpyAsync(D + o_k, k, sizeof(double) * nk, hipMemcpyHostToDevice, s);
    if (nrd && e == hipSuccess) e = hipMemcpyAsync(D + o_gn + gl.weff, weight_eff, sizeof(double) * nrd, hipMemcpyHostToDevice, s);
    if (status && e == hipSuccess) e = hipMemcpyAsync(d_stat, status, sizeof(int) * NS, hipMemcpyHostToDevice, s);
    if (nlist && e == hipSuccess) e = hipMemcpyAsync(d_srays, srays, sizeof(int) * (size_t)nlist, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
    jur_scene_gain_t q;
    memset(&q, 0, sizeof q);
    q.nslice = nslice; q.nd = nd; q.wptr = L; q.aptr = L + (NS + 1); q.sptr = L + 2 * (NS + 1); q.gptr = L + 3 * (NS + 1);
    q.koff = L + 4 * (NS + 1); q.srays = d_srays; q.status = status ? d_stat : NULL; q.S = D + o_S; q.k = D + o_k;
    q.nrd = (long)nrd; q.nb = nb;
    if ((rc = gain_enqueue(m, s, who, &q, D + o_gn, nk, ntile, ngroups, hmap, in, out, NULL))) goto done;
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; }
  }
done:
  if (enqueued && rc) (void)hipStreamSynchronize(m->stream);
  free(ptr); free(srays); free(hmap); free(hl);
  return rc;
}

/* ---- parameter errors of the slices (jur_param_slices_host) ----------------------------------------------------------- */
/* Gains and parameter blocks the caller holds.  The slab: the longs wptr | bwptr | cptr | bbptr | sptr | pptr | koff |
 * koffb, then the doubles gain | kb | weff | C | var | cov | sig, then the ints cmap | srays. */
int jur_param_slices_host(jur_model_t *m, long nslice, long const *wptr, long const *bwptr, long nr, int nd, long const *rowptr,
                          long const *rowptr_b, int const *sid, double const *gain, double const *kb, double const *weight_eff,
                          jur_param_in_t const *in, jur_param_out_t const *out) {
  char const *const who = "jur_param_slices_host";
  if (!m || nslice < 0 || nr < 0 || nd < 0) { jur_set_error("%s: bad arguments", who); return JUR_EINVAL; }
  int rc = jur_param_check_args(who, in, out);
  if (rc) return rc;
  if (nslice == 0 || nr == 0) return JUR_OK;
  if (nslice > 0x7fffffffL || nr > 0x7fffffffL) { jur_set_error("%s: at most 2^31-1 systems and rays per call", who); return JUR_EINVAL; }
  if (!wptr || !bwptr || !rowptr || !rowptr_b || !sid) {
    jur_set_error("%s: null argument (%s)", who, !wptr ? "wptr" : !bwptr ? "bwptr" : !rowptr ? "rowptr" : !rowptr_b ? "rowptr_b" : "sid");
    return JUR_EINVAL;
  }
  size_t const NS = (size_t)nslice, NR = (size_t)nr, nrd = NR * (size_t)nd, NC = (size_t)(in->nvar + in->ncov);
  long *ptr = (long *)malloc(sizeof(long) * (6 * (NS + 1) + 2 * NR));
  int *srays = (int *)malloc(sizeof(int) * NR), *hmap = NULL;
  int enqueued = 0;
  if (!ptr || !srays) { jur_set_error("%s: out of memory", who); rc = JUR_ENOMEM; goto done; }
  {
    long *const bw = ptr + NS + 1, *const cptr = bw + NS + 1, *const bbptr = cptr + NS + 1, *const sptr = bbptr + NS + 1,
         *const pptr = sptr + NS + 1, *const koff = pptr + NS + 1, *const koffb = koff + NR;
    long const nc = jur_param_layout_as(who, nslice, wptr, nr, rowptr, rowptr_b, sid, bw, cptr, bbptr);
    if (nc < 0) { rc = (int)nc; goto done; }
    if ((rc = jur_param_check_bwptr(who, nslice, bwptr, bw))) goto done;
    size_t const nk = (size_t)rowptr[nr] * (size_t)nd, nkb = (size_t)rowptr_b[nr] * (size_t)nd;
    if ((nk > 0 && !gain) || (nkb > 0 && !kb) || (nrd > 0 && !weight_eff)) {
      jur_set_error("%s: null argument (%s)", who, (nk > 0 && !gain) ? "gain" : (nkb > 0 && !kb) ? "kb" : "weight_eff");
      rc = JUR_EINVAL; goto done;
    }
    if ((rc = jur_param_check_values(who, nslice, bw, bbptr, in))) goto done;
    memcpy(ptr, wptr, sizeof(long) * (NS + 1));
    pptr[0] = 0;
    for (long q = 0; q < nslice; q++) pptr[q + 1] = pptr[q] + (wptr[q + 1] - wptr[q] + JUR_PARAM_ROWS - 1) / JUR_PARAM_ROWS;
    for (long r = 0; r < nr; r++) { koff[r] = rowptr[r] * nd; koffb[r] = rowptr_b[r] * nd; }
    long const nlist = jur_scene_rays_by_slice(nr, nslice, sid, sptr, srays);
    for (long q = 0; q < nslice; q++)
      if ((sptr[q + 1] - sptr[q]) * nd > 0x7fffffffL) {
        jur_set_error("%s: 2^31 measurements of slice %ld: call with the rays of fewer slices at a time", who, q);
        rc = JUR_EINVAL; goto done;
      }
    long const ntile = jur_param_maps(nslice, wptr, bw, NULL), ngroups = pptr[nslice];
    if (ntile > 0x7fffffffL || ngroups > 0x7fffffffL) { jur_set_error("%s: 2^31 workgroups: call with fewer systems at a time", who); rc = JUR_EINVAL; goto done; }
    if (ntile > 0) {
      hmap = (int *)malloc(sizeof(int) * 3 * (size_t)ntile);
      if (!hmap) { jur_set_error("%s: out of memory", who); rc = JUR_ENOMEM; goto done; }
      (void)jur_param_maps(nslice, wptr, bw, hmap);
    }
    size_t const nb = (size_t)wptr[nslice], nbw = (size_t)bw[nslice], nbb = (size_t)bbptr[nslice], NV = (size_t)in->nvar, NF = (size_t)in->ncov;
    size_t const nlong = 6 * (NS + 1) + 2 * NR, o_g = nlong, o_kb = o_g + nk, o_we = o_kb + nkb, o_C = o_we + nrd, o_var = o_C + (size_t)nc,
                 o_cov = o_var + NV * nbw, o_sig = o_cov + NF * nbb, o_int = o_sig + NC * nb;
    hipStream_t s;
    if ((rc = scene_slab_reserve(m, who, sizeof(double) * o_int + sizeof(int) * (3 * (size_t)ntile + (size_t)nlist + 1), &s))) goto done;
    double *const D = (double *)m->d_scene;
    long *const L = (long *)m->d_scene;
    int *const d_map = (int *)(D + o_int), *const d_srays = d_map + 3 * (size_t)ntile;
    enqueued = 1;
    hipError_t e = hipMemcpyAsync(L, ptr, sizeof(long) * nlong, hipMemcpyHostToDevice, s);
    if (nk && e == hipSuccess) e = hipMemcpyAsync(D + o_g, gain, sizeof(double) * nk, hipMemcpyHostToDevice, s);
    if (nkb && e == hipSuccess) e = hipMemcpyAsync(D + o_kb, kb, sizeof(double) * nkb, hipMemcpyHostToDevice, s);
    if (nrd && e == hipSuccess) e = hipMemcpyAsync(D + o_we, weight_eff, sizeof(double) * nrd, hipMemcpyHostToDevice, s);
    if (NV * nbw > 0 && e == hipSuccess) e = hipMemcpyAsync(D + o_var, in->var, sizeof(double) * NV * nbw, hipMemcpyHostToDevice, s);
    if (NF * nbb > 0 && e == hipSuccess) e = hipMemcpyAsync(D + o_cov, in->cov, sizeof(double) * NF * nbb, hipMemcpyHostToDevice, s);
    if (ntile && e == hipSuccess) e = hipMemcpyAsync(d_map, hmap, sizeof(int) * 3 * (size_t)ntile, hipMemcpyHostToDevice, s);
    if (nlist && e == hipSuccess) e = hipMemcpyAsync(d_srays, srays, sizeof(int) * (size_t)nlist, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
    jur_scene_param_t q;
    memset(&q, 0, sizeof q);
    q.nslice = nslice; q.nd = nd; q.nvar = in->nvar; q.ncov = in->ncov;
    q.wptr = L; q.bwptr = L + (NS + 1); q.cptr = L + 2 * (NS + 1); q.bbptr = L + 3 * (NS + 1); q.sptr = L + 4 * (NS + 1);
    q.pptr = L + 5 * (NS + 1); q.koff = L + 6 * (NS + 1); q.koffb = q.koff + NR;
    q.srays = d_srays; q.cmap = d_map; q.gain = D + o_g; q.kb = D + o_kb; q.weff = D + o_we; q.var = D + o_var; q.cov = D + o_cov;
    q.nb = (long)nb; q.nbw = (long)nbw; q.nbb = (long)nbb; q.C = D + o_C; q.sig = D + o_sig;
    if (SCENE_TIMED(m, s, jurk_scene_param(&q, ntile, ngroups, s))) { rc = launch_failed("%s: kernel launch failed", who); goto done; }
    if (nc && out->C) e = hipMemcpyAsync(out->C, q.C, sizeof(double) * (size_t)nc, hipMemcpyDeviceToHost, s);
    if (NC * nb > 0 && e == hipSuccess) e = hipMemcpyAsync(out->sigma_param, q.sig, sizeof(double) * NC * nb, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; }
  }
done:
  if (enqueued && rc) (void)hipStreamSynchronize(m->stream);
  free(ptr); free(srays); free(hmap);
  return rc;
}

/* ---- parameter errors of a scene in one call (jur_param_scene_host) --------------------------------------------------- */
/* The model's side buffer (grow-only; it holds nothing between calls): selects the device and waits for the model's earlier
 * calls as scene_slab_reserve does, which may free and grow the slab between the phases and so cannot hold what this does. */
static int scene_side_reserve(jur_model_t *m, char const *who, size_t bytes) {
  if (hipSetDevice(m->device) != hipSuccess) { jur_set_error("%s: cannot select the device", who); return JUR_EHIP; }
  int const rc = wait_done(m, m->stream);
  if (rc) return rc;
  if (bytes > m->side_bytes) {
    if (m->d_side) (void)hipFree(m->d_side);
    m->d_side = NULL; m->side_bytes = 0;
    if (hipMalloc(&m->d_side, bytes) != hipSuccess) {
      (void)hipGetLastError(); jur_set_error("%s: no device memory for %zu bytes", who, bytes); return JUR_ENOMEM;
    }
    m->side_bytes = bytes;
  }
  return JUR_OK;
}

/* The side buffer: the longs wptr | bwptr | cptr | bbptr | sptr | pptr | koff | koffb, then the doubles gain | weff | C |
 * var | cov | sig, then the ints pmap (the tiles of one pass) | srays.  The model's windows are the caller's to put back. */
static int param_scene_body(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double *rad, double *tau,
                            double *const tp[3], int *np_out, long const *rowptr, double const *y, double const *weight,
                            double const *prior_ivar, jur_diag_out_t const *diag, jur_gain_in_t const *gin, jur_gain_out_t const *gout,
                            jur_param_scene_in_t const *pin, jur_param_scene_out_t const *pout,
                            double *A, double *b, double *cost, long *nlive, double *k, long max_rays_per_pass) {
  char const *const who = "jur_param_scene_host";
  { int const ri = scene_ip_check(m, who); if (ri) return ri; }
  if (nr < 0 || max_rays_per_pass < 0) { jur_set_error("%s: bad arguments", who); return JUR_EINVAL; }
  int rc = jur_param_check_args(who, pin->in, pout->out);
  if (rc) return rc;
  if (!pin->ctl_b || !pin->rowptr_b) { jur_set_error("%s: null argument (%s)", who, !pin->ctl_b ? "ctl_b" : "rowptr_b"); return JUR_EINVAL; }
  int const nd = m->ctl->nd, ng = m->view.ng, nw = m->view.nw;
  if ((rc = ret_windows_check(who, ng, nw, pin->ctl_b))) return rc;
  if ((rc = scene_atm_check(m, who, "every p, T or H2O element moves every pressure and the Jacobian has no blocks: use jur_kernel", atm))) return rc;
  if (nr == 0) return JUR_OK;
  if (nr > 0x7fffffffL) { jur_set_error("%s: at most 2^31-1 rays per call", who); return JUR_EINVAL; }
  if (!geom || !rad || !tau || !tp || !rowptr) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  jur_param_in_t const *const in = pin->in;
  jur_param_out_t const *const out = pout->out;
  size_t const NR = (size_t)nr, nrd = NR * (size_t)nd, NC = (size_t)(in->nvar + in->ncov), nrow = 6 + (size_t)ng + nw;
  int *first = (int *)malloc(sizeof(int) * 4 * NR), *len = first ? first + NR : NULL, *sid = len ? len + NR : NULL, *srays = sid ? sid + NR : NULL;
  long *rp = (long *)malloc(sizeof(long) * 2 * (NR + 1)), *rpb = rp ? rp + NR + 1 : NULL, *ptr = NULL, *mark = NULL;
  ctl_t *cb = (ctl_t *)malloc(sizeof(ctl_t));
  jur_scene_slice_t *sl = NULL, *slb = NULL;
  double *hrad = NULL;                              /* the input mask, then the outputs of phase 2 that nobody reads: rad | tau | tp */
  int *hmap = NULL;
  int enqueued = 0;
  if (!first || !rp || !cb) { jur_set_error("%s: out of memory", who); rc = JUR_ENOMEM; goto done; }
  /* the two layouts: the retrieved state under the model's windows, the parameters under ctl_b's */
  if ((rc = jur_scene_layout(m->ctl, atm, nr, geom[0], first, len, rp))) goto done;
  if (memcmp(rp, rowptr, sizeof(long) * (NR + 1))) {
    jur_set_error("%s: rowptr is not jur_scene_layout's for these rays, this atmosphere and these windows", who);
    rc = JUR_EINVAL; goto done;
  }
  long const nslice = jur_scene_distinct(atm->np, nr, first, len, rp, sid, &sl);
  if (nslice < 0) { jur_set_error("%s: out of memory", who); rc = JUR_ENOMEM; goto done; }
  memcpy(cb, m->ctl, sizeof(ctl_t));
  ret_windows_copy(cb, pin->ctl_b, ng, nw);
  if ((rc = jur_scene_layout(cb, atm, nr, geom[0], first, len, rpb))) goto done;
  if (memcmp(rpb, pin->rowptr_b, sizeof(long) * (NR + 1))) {
    jur_set_error("%s: rowptr_b is not jur_scene_layout's for these rays, this atmosphere and the windows of ctl_b", who);
    rc = JUR_EINVAL; goto done;
  }
  size_t const NS = (size_t)nslice, nlong = 6 * (NS + 1) + 2 * NR;
  ptr = (long *)calloc(nlong, sizeof(long));
  mark = (long *)calloc(NS ? NS : 1, sizeof(long));
  hrad = (double *)malloc(sizeof(double) * (2 * nrd + 3 * NR));
  if (!ptr || !mark || !hrad) { jur_set_error("%s: out of memory", who); rc = JUR_ENOMEM; goto done; }
  {
    long *const wptr = ptr, *const bw = wptr + NS + 1, *const cptr = bw + NS + 1, *const bbptr = cptr + NS + 1, *const sptr = bbptr + NS + 1,
         *const pptr = sptr + NS + 1, *const koff = pptr + NS + 1, *const koffb = koff + NR;
    for (long q = 0; q < nslice; q++) {
      wptr[q + 1] = wptr[q] + sl[q].nel;
      pptr[q + 1] = pptr[q] + (sl[q].nel + JUR_PARAM_ROWS - 1) / JUR_PARAM_ROWS;
    }
    long const nc = jur_param_layout_as(who, nslice, wptr, nr, rp, rpb, sid, bw, cptr, bbptr);
    if (nc < 0) { rc = (int)nc; goto done; }
    if (pin->bwptr && (rc = jur_param_check_bwptr(who, nslice, pin->bwptr, bw))) goto done;
    if ((rc = jur_param_check_values(who, nslice, bw, bbptr, in))) goto done;
    for (long r = 0; r < nr; r++) { koff[r] = rp[r] * nd; koffb[r] = rpb[r] * nd; }
    long const nlist = jur_scene_rays_by_slice(nr, nslice, sid, sptr, srays);
    for (long q = 0; q < nslice; q++)
      if ((sptr[q + 1] - sptr[q]) * nd > 0x7fffffffL) {
        jur_set_error("%s: 2^31 measurements of slice %ld: call with the rays of fewer slices at a time", who, q);
        rc = JUR_EINVAL; goto done;
      }
    long const ntile = jur_param_maps(nslice, wptr, bw, NULL), ngroups = pptr[nslice];
    if (ntile > 0x7fffffffL / 5 || ngroups > 0x7fffffffL) { jur_set_error("%s: 2^31 workgroups: call with the rays of fewer slices at a time", who); rc = JUR_EINVAL; goto done; }
    size_t const nk = (size_t)rp[nr] * (size_t)nd, nb = (size_t)wptr[nslice], nbw = (size_t)bw[nslice], nbb = (size_t)bbptr[nslice],
                 NV = (size_t)in->nvar, NF = (size_t)in->ncov;
    size_t const o_g = nlong, o_we = o_g + nk, o_C = o_we + nrd, o_var = o_C + (size_t)nc, o_cov = o_var + NV * nbw, o_sig = o_cov + NF * nbb,
                 o_int = o_sig + NC * nb;
    size_t const side_bytes = sizeof(double) * o_int + sizeof(int) * (5 * (size_t)ntile + (size_t)nlist + 1);
    /* what phase 2 stacks under ctl_b's windows is known here: both phases are refused before the first is launched */
    long const nsb = jur_scene_distinct(atm->np, nr, first, len, rpb, srays, &slb);   /* (srays: scratch until the lists are made again below) */
    if (nsb < 0) { jur_set_error("%s: out of memory", who); rc = JUR_ENOMEM; goto done; }
    double ntb = (double)atm->np;
    for (long q = 0; q < nsb; q++) ntb += (double)slb[q].nel * (double)slb[q].len;
    double const atm_b_bytes = sizeof(double) * (double)(nrow + 1) * ntb;
    if ((double)side_bytes + atm_b_bytes > (double)(m->ws_budget / 2)) {
      jur_set_error("%s: the gain, the effective weights, C and the parameter covariances (%zu bytes) do not fit beside the atmosphere "
                    "stacked under the windows of ctl_b (%.0f bytes) in the workspace budget: call with the rays of fewer slices at a time",
                    who, side_bytes, atm_b_bytes);
      rc = JUR_ENOMEM; goto done;
    }
    (void)jur_scene_rays_by_slice(nr, nslice, sid, sptr, srays);
    if (ntile > 0 && !(hmap = (int *)malloc(sizeof(int) * 5 * (size_t)ntile))) { jur_set_error("%s: out of memory", who); rc = JUR_ENOMEM; goto done; }
    memcpy(hrad, rad, sizeof(double) * nrd);
    if ((rc = scene_side_reserve(m, who, side_bytes))) goto done;
    double *const D = (double *)m->d_side;
    long *const L = (long *)m->d_side;
    int *const d_pmap = (int *)(D + o_int), *const d_srays = d_pmap + 5 * (size_t)ntile;
    hipStream_t const s = m->stream;

    /* phase 1: the body of jur_gain_scene_host; the gain and the effective weights stay in the side buffer */
    scene_normal_t const nm = {y, weight, A, b, cost, nlive};
    scene_diag_t const dg = {prior_ivar, diag, gin, gout};
    scene_param_t pm;
    memset(&pm, 0, sizeof pm);
    pm.phase = 1; pm.bytes = side_bytes; pm.gain = D + o_g; pm.weff = D + o_we;
    if ((rc = kernel_scene_body(m, atm, nr, geom, rad, tau, tp, np_out, rowptr, k, max_rays_per_pass, &nm, NULL, NULL, &dg, NULL, &pm, who))) goto done;
    enqueued = 1;
    hipError_t e = hipSuccess;
    if (pout->weight_eff) {
      /* jurk_scene_weff does not look at the slices (a ray without one is in no list): such a ray's measurements are
       * not live, and the array that goes home says so */
      if (nslice > 0) e = hipMemcpyAsync(pout->weight_eff, pm.weff, sizeof(double) * nrd, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      for (long r = 0; r < nr && e == hipSuccess; r++)
        if (sid[r] < 0) memset(pout->weight_eff + (size_t)r * (size_t)nd, 0, sizeof(double) * (size_t)nd);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(L, ptr, sizeof(long) * nlong, hipMemcpyHostToDevice, s);
    if (NV * nbw > 0 && e == hipSuccess) e = hipMemcpyAsync(D + o_var, in->var, sizeof(double) * NV * nbw, hipMemcpyHostToDevice, s);
    if (NF * nbb > 0 && e == hipSuccess) e = hipMemcpyAsync(D + o_cov, in->cov, sizeof(double) * NF * nbb, hipMemcpyHostToDevice, s);
    if (nlist && e == hipSuccess) e = hipMemcpyAsync(d_srays, srays, sizeof(int) * (size_t)nlist, hipMemcpyHostToDevice, s);
    if (nc && e == hipSuccess) e = hipMemsetAsync(D + o_C, 0, sizeof(double) * (size_t)nc, s);   /* (every chain starts from +0.0) */
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
    jur_scene_param_t *const q = &pm.q;
    q->nslice = nslice; q->nd = nd; q->nvar = in->nvar; q->ncov = in->ncov;
    q->wptr = L; q->bwptr = L + (NS + 1); q->cptr = L + 2 * (NS + 1); q->bbptr = L + 3 * (NS + 1); q->sptr = L + 4 * (NS + 1);
    q->pptr = L + 5 * (NS + 1); q->koff = L + 6 * (NS + 1); q->koffb = q->koff + NR;
    q->srays = d_srays; q->gain = D + o_g; q->weff = D + o_we; q->var = D + o_var; q->cov = D + o_cov;
    q->nb = (long)nb; q->nbw = (long)nbw; q->nbb = (long)nbb; q->C = D + o_C; q->sig = D + o_sig;

    /* phase 2: the Jacobian passes under ctl_b's windows, the chains of C continued after each; rad (the input mask),
     * tau and tp of this call are the forward model's once more and go nowhere */
    if (ntile > 0 || pout->kb) {
      pm.phase = 2; pm.wptr = wptr; pm.bwptr = bw; pm.sptr = sptr; pm.srays = srays; pm.sid = sid; pm.mark = mark; pm.hmap = hmap; pm.d_pmap = d_pmap;
      double *const tp2[3] = {hrad + 2 * nrd, hrad + 2 * nrd + NR, hrad + 2 * nrd + 2 * NR};
      ret_windows_copy(m->ctl, pin->ctl_b, ng, nw);
      if ((rc = kernel_scene_body(m, atm, nr, geom, hrad, hrad + nrd, tp2, NULL, rpb, pout->kb, max_rays_per_pass, NULL, NULL, NULL, NULL, NULL, &pm, who))) goto done;
    }

    /* phase 3: the quadratic forms on the finished C; what was asked for comes home */
    if (NC * nb > 0) {
      if (SCENE_TIMED(m, s, jurk_scene_param(q, 0, ngroups, s))) { rc = launch_failed("%s: kernel launch failed", who); goto done; }
    }
    if (nc && out->C) e = hipMemcpyAsync(out->C, q->C, sizeof(double) * (size_t)nc, hipMemcpyDeviceToHost, s);
    if (NC * nb > 0 && e == hipSuccess) e = hipMemcpyAsync(out->sigma_param, q->sig, sizeof(double) * NC * nb, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    enqueued = 0;
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; }
  }
done:
  if (enqueued) (void)hipStreamSynchronize(m->stream);   /* copies out of the arrays freed here may still be under way */
  free(first); free(rp); free(ptr); free(mark); free(cb); free(sl); free(slb); free(hrad); free(hmap);
  return rc;
}

int jur_param_scene_host(jur_model_t *m, atm_t const *atm, long nr, double const *const geom[7], double *rad, double *tau,
                         double *const tp[3], int *np_out, long const *rowptr, double const *y, double const *weight,
                         double const *prior_ivar, jur_diag_out_t const *diag, jur_gain_in_t const *gin, jur_gain_out_t const *gout,
                         jur_param_scene_in_t const *pin, jur_param_scene_out_t const *pout,
                         double *A, double *b, double *cost, long *nlive, double *k, long max_rays_per_pass) {
  if (!m || !atm || !gin || !gout || !pin || !pout) { jur_set_error("jur_param_scene_host: null argument"); return JUR_EINVAL; }
  ctl_t *own = (ctl_t *)malloc(sizeof(ctl_t));      /* the model's own windows, in force again whatever happens */
  if (!own) { jur_set_error("jur_param_scene_host: out of memory"); return JUR_ENOMEM; }
  ret_windows_copy(own, m->ctl, m->view.ng, m->view.nw);
  int const rc = param_scene_body(m, atm, nr, geom, rad, tau, tp, np_out, rowptr, y, weight, prior_ivar, diag, gin, gout, pin, pout,
                                  A, b, cost, nlive, k, max_rays_per_pass);
  ret_windows_copy(m->ctl, own, m->view.ng, m->view.nw);
  free(own);
  return scene_restore_atm(m, atm, rc);
}

/* The upstream parametrisation of the prior, built and inverted on the device.  The slab of the scene entries serves:
 * wptr | aptr, z | sigma | cz | zeros (the solve's b) | live | dx | lam (zeros) | pred, Sa | L | R, then the ints
 * iq | status | imap. */
int jur_prior_corr_host(jur_model_t *m, long nslice, long const *wptr, int const *iq, double const *z, double const *sigma,
                        int nq, double const *cz, double *R, double *Sa, int *status) {
  char const *const who = "jur_prior_corr_host";
  if (!m || nslice < 0) { jur_set_error("%s: bad arguments", who); return JUR_EINVAL; }
  if (nslice == 0) return JUR_OK;
  if (nslice > 0x7fffffffL) { jur_set_error("%s: at most 2^31-1 systems per call", who); return JUR_EINVAL; }
  if (!wptr || !R || !status) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  int rc = jur_prior_check_corr(who, nslice, wptr, iq, z, sigma, nq, cz);
  if (rc) return rc;
  size_t const NS = (size_t)nslice, NQ = (size_t)nq;
  long *ptr = (long *)malloc(sizeof(long) * 2 * (NS + 1)), *aptr = ptr ? ptr + NS + 1 : NULL;
  int *hmap = NULL;
  long ninv = 0, ntile = 0;
  if (!ptr) return JUR_ENOMEM;
  int enqueued = 0;
  memcpy(ptr, wptr, sizeof(long) * (NS + 1));
  aptr[0] = 0;
  for (long q = 0; q < nslice; q++) { long const w = wptr[q + 1] - wptr[q]; aptr[q + 1] = aptr[q] + w * w; }
  if ((rc = diag_maps_make(who, nslice, wptr, &ninv, &ntile, &hmap))) goto done;
  {
    size_t const NA = (size_t)aptr[nslice], NB = (size_t)wptr[nslice];
    size_t const o_z = 2 * (NS + 1), o_sig = o_z + NB, o_cz = o_sig + NB, o_zero = o_cz + NQ, o_live = o_zero + NB, o_dx = o_live + NB,
                 o_lam = o_dx + NB, o_pred = o_lam + NS, o_Sa = o_pred + NS, o_L = o_Sa + NA, o_R = o_L + NA, o_int = o_R + NA;
    size_t const bytes = sizeof(double) * o_int + sizeof(int) * (NB + NS + 2 * (size_t)ninv + 1);
    hipStream_t s;
    if ((rc = scene_slab_reserve(m, who, bytes, &s))) goto done;
    double *const D = (double *)m->d_scene;
    long *const L = (long *)m->d_scene;
    int *const d_iq = (int *)(D + o_int), *const d_stat = d_iq + NB, *const d_imap = d_stat + NS;
    enqueued = 1;
    hipError_t e = hipMemcpyAsync(L, ptr, sizeof(long) * 2 * (NS + 1), hipMemcpyHostToDevice, s);
    if (NB && e == hipSuccess) e = hipMemcpyAsync(D + o_z, z, sizeof(double) * NB, hipMemcpyHostToDevice, s);
    if (NB && e == hipSuccess) e = hipMemcpyAsync(D + o_sig, sigma, sizeof(double) * NB, hipMemcpyHostToDevice, s);
    if (NQ && e == hipSuccess) e = hipMemcpyAsync(D + o_cz, cz, sizeof(double) * NQ, hipMemcpyHostToDevice, s);
    if (NB && e == hipSuccess) e = hipMemcpyAsync(d_iq, iq, sizeof(int) * NB, hipMemcpyHostToDevice, s);
    if (NB && e == hipSuccess) e = hipMemsetAsync(D + o_zero, 0, sizeof(double) * NB, s);
    if (e == hipSuccess) e = hipMemsetAsync(D + o_lam, 0, sizeof(double) * NS, s);
    if (ninv > 0 && e == hipSuccess) e = hipMemcpyAsync(d_imap, hmap, sizeof(int) * 2 * (size_t)ninv, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; goto done; }
    jur_scene_pcov_t c;
    memset(&c, 0, sizeof c);
    c.nslice = nslice; c.wptr = L; c.aptr = L + NS + 1; c.iq = d_iq; c.z = D + o_z; c.sigma = D + o_sig; c.nq = nq; c.cz = D + o_cz;
    c.Sa = D + o_Sa;
    jur_scene_solve_t q;
    memset(&q, 0, sizeof q);
    q.nslice = nslice; q.wptr = c.wptr; q.aptr = c.aptr; q.A = c.Sa; q.b = D + o_zero; q.mode = JUR_DAMP_MARQUARDT;
    q.M = D + o_L; q.live = D + o_live; q.lam = D + o_lam; q.dx = D + o_dx; q.pred = D + o_pred; q.status = d_stat;
    jur_scene_diag_t d;
    memset(&d, 0, sizeof d);
    d.nslice = nslice; d.wptr = c.wptr; d.aptr = c.aptr; d.A = c.Sa; d.L = q.M; d.live = q.live; d.status = d_stat; d.imap = d_imap;
    d.S = D + o_R;
    int const ti = scene_timed_begin(m, s);
    int ek = jurk_scene_prior_cov(&c, (long)NA, s);
    if (!ek) ek = jurk_scene_solve(&q, s);
    if (!ek) ek = jurk_scene_prior_inverse(&d, ninv, s);
    scene_timed_end(m, ti, s);
    if (ek) { jur_set_error("%s: kernel launch failed", who); rc = JUR_EHIP; goto done; }
    if (NA) e = hipMemcpyAsync(R, d.S, sizeof(double) * NA, hipMemcpyDeviceToHost, s);
    if (NA && Sa && e == hipSuccess) e = hipMemcpyAsync(Sa, c.Sa, sizeof(double) * NA, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(status, d_stat, sizeof(int) * NS, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { jur_set_error("%s: %s", who, hipGetErrorString(e)); rc = JUR_EHIP; }
  }
done:
  if (enqueued && rc) (void)hipStreamSynchronize(m->stream);
  free(ptr); free(hmap);
  return rc;
}

/* ---- drop-in entry points ------------------------------------------------------ */
#define DIE(...)                                                                 \
  do {                                                                           \
    printf("\nError (%s, %s, l%d): ", __FILE__, __func__, __LINE__);             \
    printf(__VA_ARGS__);                                                         \
    printf("\n\n");                                                              \
    fflush(stdout);                                                              \
    exit(EXIT_FAILURE);                                                          \
  } while (0)

/* The reference serves concurrent callers (OpenMP threads) through up to 4 "lanes", each with its own
 * stream and buffers (GPUdrivers.cu:262-342).  Same idea here: lane 0 is the process-lifetime model that
 * owns the tables (like upstream's static tbl), further lanes are created on demand as shallow copies that
 * share the table arrays and own their atmosphere, workspace and stream.  A small package (<= 1088 rays)
 * leaves most of the GPU idle, so concurrent packages overlap almost perfectly. */
#define JUR_MAX_LANES 16
static pthread_mutex_t g_lock = PTHREAD_MUTEX_INITIALIZER;
static pthread_cond_t g_cond = PTHREAD_COND_INITIALIZER;
static jur_model_t *g_lane[JUR_MAX_LANES];   /* g_lane[0]: owner of the tables */
static int g_busy[JUR_MAX_LANES];
static int g_nlane = 0, g_maxlane = 0;

static jur_model_t *clone_lane(jur_model_t const *m) {
  jur_model_t *c = (jur_model_t *)malloc(sizeof *c);
  if (!c) return NULL;
  *c = *m;
  c->shared_tables = 1;
  c->ctl = (ctl_t *)malloc(sizeof(ctl_t));
  if (!c->ctl) { free(c); return NULL; }
  memcpy(c->ctl, m->ctl, sizeof(ctl_t));
  c->d_atm = NULL; c->atm_cap = 0; c->atm_slices = 0; c->atm_k_zero = 0; c->view.atm_k_zero = 0;
  c->view.atm_np = 0;
  c->d_track = NULL; c->track_bytes = 0; c->track.nprof = 0;
  c->d_cloud = NULL; c->cloud_bytes = 0; c->cloud.np = 0; c->cloud.x1 = NULL;
  c->d_los = NULL; c->d_eps = NULL; c->d_np = NULL; c->d_tsurf = NULL; c->d_status = NULL;
  c->los_bytes = 0; c->ws_rays = 0; c->ws_trace_rays = 0;
  c->d_order = NULL; c->d_sort_tmp = NULL; c->d_blk_order = NULL; c->order_cap = 0; c->sort_tmp_bytes = 0; c->n_blk_order = 0;
  c->d_io = NULL; c->d_io_np = NULL; c->io_cap = 0;
  c->h_io = NULL; c->h_io_cap = 0; c->h_pkg = NULL; c->h_atm = NULL; c->h_atm_n = 0; c->h_atm_cap = 0; c->h_status = NULL;
  c->stream = NULL; c->stream2 = NULL; c->ev_mask = NULL; c->ev_trace = NULL;
  c->host_call = 0; c->have_done = 0; c->ev_done = NULL; c->d_fov = NULL; c->fov_cap = 0; c->fov_n = 0; c->fov_shape = NULL; c->d_fov_shape = NULL; c->pp_nslice = 0; c->pp_wptr = NULL; c->pp_R = NULL; c->d_pp = NULL; c->d_kq = NULL; c->h_kq = NULL; c->kq_cap = 0;
  c->d_ctb = NULL; c->ctb_cap = 0; c->d_side = NULL; c->side_bytes = 0;
  c->timing = 0; c->evpool = NULL; c->evkind = NULL; c->ntimed = 0;
  if (hipSetDevice(c->device) != hipSuccess || create_streams(c) != JUR_OK ||
      hipMalloc((void **)&c->d_status, sizeof(int)) != hipSuccess || hipMemset(c->d_status, 0, sizeof(int)) != hipSuccess) {
    jur_model_destroy(c);
    return NULL;
  }
  return c;
}

/* run-time switches of the control block are honoured on every call (upstream re-uploads ctl per call,
 * GPUdrivers.cu:355); nu/emitter/tables are latched by the first call (jr_common.h:62-63) */
static void refresh_switches(jur_model_t *m, ctl_t const *ctl) {
  jur_view_t *v = &m->view;
  if (ctl->ng != v->ng || ctl->nd != v->nd) DIE("ng/nd changed after the tables were initialised");
  if (ctl->ip != 1 && ctl->ip != 2 && ctl->ip != 3) DIE("IP %d is not supported along the line of sight (1: profile, 2: satellite track, 3: point cloud)", ctl->ip);
  if (ctl->ip == 3 && !(ctl->cx > 0 && isfinite(ctl->cx) && ctl->cz > 0 && isfinite(ctl->cz))) DIE("IP 3 needs finite CX > 0 and CZ > 0 (cx = %g, cz = %g)", ctl->cx, ctl->cz);
  /* the next set_atm builds the profile table or the position table (the influence lengths travel with it) */
  if (ctl->ip != m->track.ip || (ctl->ip == 3 && (ctl->cx != m->cloud.cx || ctl->cz != m->cloud.cz))) {
    m->track.ip = ctl->ip; m->track.nprof = 0; m->cloud.np = 0; m->cloud.cx = ctl->cx; m->cloud.cz = ctl->cz; m->h_atm_n = 0;
  }
  memcpy(m->ctl, ctl, sizeof(ctl_t));
  v->refrac = ctl->refrac; v->write_bbt = ctl->write_bbt; v->rayds = ctl->rayds; v->raydz = ctl->raydz;
  /* upstream looks the emitters up on the first call that has the switch on, whichever call that is
   * (CPUdrivers.c:126-128: `if (ctl->ctm_h2o && -999 == ig_h2o) ig_h2o = find_emitter(...)`) */
  if (ctl->ctm_h2o && v->ig_h2o == -999) { v->ig_h2o = find_emitter(ctl, "H2O"); m->h_atm_n = 0; }   /* hydrostatic uses it */
  if (ctl->ctm_co2 && v->ig_co2 == -999) v->ig_co2 = find_emitter(ctl, "CO2");
  v->fourbit = ((1 == ctl->ctm_co2) && (v->ig_co2 >= 0)) * 8 + ((1 == ctl->ctm_h2o) && (v->ig_h2o >= 0)) * 4
             + (1 == ctl->ctm_n2) * 2 + (1 == ctl->ctm_o2) * 1;
}

/* returns a lane index marked busy; blocks while all lanes are in use */
static int acquire_lane(ctl_t const *ctl) {
  pthread_mutex_lock(&g_lock);
  if (g_nlane == 0) {   /* first call of the process: load the tables (upstream: get_tbl under omp critical) */
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
      DIE("no GPU found: this library has no CPU path (USEGPU = %d)", ctl->useGPU);
    int device = ctl->MPIlocalrank;               /* GPUdrivers.cu:344 */
    if (device < 0 || device >= ndev) device = 0;
    printf("Initialize emissivity tables and source function (MI355X path, device %d)...\n", device);
    if (jur_model_create_from_files(&g_lane[0], ctl, device) != JUR_OK) DIE("%s", jur_last_error());
    g_nlane = 1;
    char const *e = getenv("JUR_LANES");
    g_maxlane = e ? atoi(e) : 4;
    if (g_maxlane < 1) g_maxlane = 1;
    if (g_maxlane > JUR_MAX_LANES) g_maxlane = JUR_MAX_LANES;
  }
  int lane = -1;
  for (;;) {
    for (int i = 0; i < g_nlane && lane < 0; i++)
      if (!g_busy[i]) lane = i;
    if (lane < 0 && g_nlane < g_maxlane) {
      g_lane[g_nlane] = clone_lane(g_lane[0]);
      if (!g_lane[g_nlane]) DIE("cannot create another lane: %s", jur_last_error());
      lane = g_nlane++;
    }
    if (lane >= 0) break;
    pthread_cond_wait(&g_cond, &g_lock);
  }
  g_busy[lane] = 1;
  pthread_mutex_unlock(&g_lock);
  refresh_switches(g_lane[lane], ctl);
  return lane;
}

static void release_lane(int lane) {
  pthread_mutex_lock(&g_lock);
  g_busy[lane] = 0;
  pthread_cond_signal(&g_cond);
  pthread_mutex_unlock(&g_lock);
}

static void formod_range(ctl_t const *ctl, atm_t *atm, obs_t *obs, int r0, int nr) {
  if (ctl->checkmode) { printf("# %s: no operation in checkmode\n", __func__); return; }
  if (!obs || !atm) DIE("null argument");
  if (r0 < 0 || nr < 0 || r0 + nr > JUR_NR) DIE("ray range outside the package (max %d rays)", JUR_NR);
  if (nr == 0) return;
  int const lane = acquire_lane(ctl);
  jur_model_t *m = g_lane[lane];
  if (jur_model_set_atm(m, atm) != JUR_OK) DIE("%s", jur_last_error());
  int const nd = ctl->nd;
  if (!m->h_pkg && hipHostMalloc((void **)&m->h_pkg, sizeof(double) * 2 * JUR_NR * (size_t)nd, hipHostMallocDefault) != hipSuccess)
    DIE("Out of memory!");
  double *const buf = m->h_pkg;                  /* the lane's package scratch, kept for the life of the process */
  double *rad = buf, *tau = buf + (size_t)nr * nd;
  for (int i = 0; i < nr; i++)
    for (int id = 0; id < nd; id++) rad[(size_t)i * nd + id] = obs->rad[r0 + i][id];
  double const *geom[7] = {obs->time + r0, obs->obsz + r0, obs->obslon + r0, obs->obslat + r0,
                           obs->vpz + r0, obs->vplon + r0, obs->vplat + r0};
  double *tp[3] = {obs->tpz + r0, obs->tplon + r0, obs->tplat + r0};
  int const rc = jur_formod_host(m, nr, geom, rad, tau, tp, NULL);
  if (rc == JUR_ENLOS) DIE("Too many LOS points!");
  if (rc != JUR_OK) DIE("%s", jur_last_error());
  for (int i = 0; i < nr; i++) {
    for (int id = 0; id < nd; id++) {
      obs->rad[r0 + i][id] = rad[(size_t)i * nd + id];
      obs->tau[r0 + i][id] = tau[(size_t)i * nd + id];
    }
    for (int id = nd; id < JUR_ND; id++) {          /* upstream clears all ND channels, CPUdrivers.c:58-60 */
      obs->rad[r0 + i][id] = 0.0;
      obs->tau[r0 + i][id] = 1.0;
    }
  }
  release_lane(lane);
}

/* Explicit finalize for the drop-in entry's process-global state (upstream never frees its own,
 * GPUdrivers.cu:263-273, 309): every lane with its stream, atmosphere, workspace and pinned images, and the tables
 * of lane 0.  Waits for lanes that are still in a call.  A later formod() initialises again from the files named
 * by its ctl.  Safe to call twice, before any formod(), and from an atexit handler. */
int jur_dropin_finalize(void) {
  pthread_mutex_lock(&g_lock);
  for (int i = 0; i < g_nlane; i++)
    while (g_busy[i]) pthread_cond_wait(&g_cond, &g_lock);
  int const n = g_nlane;
  for (int i = n - 1; i >= 0; i--) {              /* lane 0 owns the tables the others share: last */
    if (g_lane[i]) {
      (void)hipSetDevice(g_lane[i]->device);
      if (g_lane[i]->stream) (void)hipStreamSynchronize(g_lane[i]->stream);
      jur_model_destroy(g_lane[i]);
    }
    g_lane[i] = NULL;
  }
  g_nlane = 0;
  g_maxlane = 0;
  pthread_mutex_unlock(&g_lock);
  return n;
}

void formod_GPU(ctl_t const *ctl, atm_t *atm, obs_t *obs) { formod_range(ctl, atm, obs, 0, obs ? obs->nr : 0); }

void formod(ctl_t const *ctl, atm_t *atm, obs_t *obs) {
  if (ctl->checkmode)
    printf("# %s: %d max %d rays , %d of max %d gases, %d of max %d channels\n", __func__, obs->nr, JUR_NR, ctl->ng,
           JUR_NG, ctl->nd, JUR_ND);
  /* USEGPU = 0 ("never") has no meaning here: every path is the GPU path. */
  formod_GPU(ctl, atm, obs);
}

void formod_pencil(ctl_t const *ctl, atm_t *atm, obs_t *obs, int const ir) { formod_range(ctl, atm, obs, ir, 1); }

/* formod() and the contribution of every emitter in one call (formod TASK contrib): obs as formod() leaves it,
 * contrib[g] (g < ng) the spectrum of emitter g alone, contrib[ng] that of the extinction alone; each gets obs's
 * geometry and tangent points (jur_formod_contrib_host). */
void formod_contrib(ctl_t const *ctl, atm_t *atm, obs_t *obs, obs_t *contrib) {
  if (ctl->checkmode) { printf("# %s: no operation in checkmode\n", __func__); return; }
  if (!obs || !atm || !contrib) DIE("null argument");
  int const nr = obs->nr, nd = ctl->nd, nv = ctl->ng + 1;
  if (nr < 0 || nr > JUR_NR) DIE("ray count outside the package (max %d rays)", JUR_NR);
  for (int v = 0; v < nv; v++) contrib[v].nr = nr;
  if (nr == 0) return;
  int const lane = acquire_lane(ctl);
  jur_model_t *m = g_lane[lane];
  if (jur_model_set_atm(m, atm) != JUR_OK) DIE("%s", jur_last_error());
  size_t const nrd = (size_t)nr * nd;
  double *const buf = (double *)malloc(sizeof(double) * (2 + 2 * (size_t)nv) * nrd);
  if (!buf) DIE("Out of memory!");
  double *const rad = buf, *const tau = rad + nrd, *const rad_c = tau + nrd, *const tau_c = rad_c + nv * nrd;
  for (int i = 0; i < nr; i++)
    for (int id = 0; id < nd; id++) rad[(size_t)i * nd + id] = obs->rad[i][id];
  double const *geom[7] = {obs->time, obs->obsz, obs->obslon, obs->obslat, obs->vpz, obs->vplon, obs->vplat};
  double *tp[3] = {obs->tpz, obs->tplon, obs->tplat};
  int const rc = jur_formod_contrib_host(m, nr, geom, rad, tau, tp, NULL, rad_c, tau_c);
  if (rc == JUR_ENLOS) DIE("Too many LOS points!");
  if (rc != JUR_OK) DIE("%s", jur_last_error());
  for (int v = -1; v < nv; v++) {                 /* v = -1: obs itself */
    obs_t *const o = (v < 0) ? obs : &contrib[v];
    double const *const r = (v < 0) ? rad : rad_c + (size_t)v * nrd, *const t = (v < 0) ? tau : tau_c + (size_t)v * nrd;
    if (v >= 0) {
      memcpy(o->time, obs->time, sizeof(double) * nr);
      memcpy(o->obsz, obs->obsz, sizeof(double) * nr);
      memcpy(o->obslon, obs->obslon, sizeof(double) * nr);
      memcpy(o->obslat, obs->obslat, sizeof(double) * nr);
      memcpy(o->vpz, obs->vpz, sizeof(double) * nr);
      memcpy(o->vplon, obs->vplon, sizeof(double) * nr);
      memcpy(o->vplat, obs->vplat, sizeof(double) * nr);
      memcpy(o->tpz, obs->tpz, sizeof(double) * nr);
      memcpy(o->tplon, obs->tplon, sizeof(double) * nr);
      memcpy(o->tplat, obs->tplat, sizeof(double) * nr);
    }
    for (int i = 0; i < nr; i++) {
      for (int id = 0; id < nd; id++) {
        o->rad[i][id] = r[(size_t)i * nd + id];
        o->tau[i][id] = t[(size_t)i * nd + id];
      }
      for (int id = nd; id < JUR_ND; id++) { o->rad[i][id] = 0.0; o->tau[i][id] = 1.0; }
    }
  }
  free(buf);
  release_lane(lane);
}

/* kernel() under its own name (jurassic.h:664, jurassic.c:812-857): the Jacobian into a gsl_matrix of
 * (finite measurements) x (state elements).  GSL is not a dependency of this library: jur_gsl_matrix_t restates the
 * layout of gsl_matrix (include/jurassic_hip.h).  obs returns the unperturbed forward model, as upstream. */
void kernel(ctl_t const *ctl, atm_t *atm, obs_t *obs, jur_gsl_matrix_t *k) {
  if (!ctl || !atm || !obs || !k || !k->data) DIE("null argument");
  if (ctl->checkmode) { printf("# %s: no operation in checkmode\n", __func__); return; }
  if (k->tda < k->size2) DIE("matrix with tda < size2");
  int const lane = acquire_lane(ctl);
  jur_model_t *m = g_lane[lane];
  /* (upstream sizes the matrix from obs2y / atm2x of the caller's obs and atm before the call, retrieval.c; so does the caller here) */
  int const rc = kernel_ld(m, atm, obs, k->data, k->size1, k->size2, k->tda);
  if (rc == JUR_ENLOS) DIE("Too many LOS points!");
  if (rc != JUR_OK) DIE("%s", jur_last_error());
  release_lane(lane);
}
