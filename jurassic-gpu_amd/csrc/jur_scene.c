/* jur_scene.c -- layout of the block Jacobian of a scene (jur_kernel_scene_host) and of its normal equations
 * (jur_normal_scene_host): which slice of the atmosphere every ray is traced through, which state elements lie in it
 * and which distinct slices a scene has.  Host arithmetic only: no GPU, no model. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include "jur_internal.h"

/* locate_atm (jr_common.h:127-154): the slice [*first, *first + return) of the n points with time stamps `time` that
 * a ray with time stamp t is traced through */
int jur_atm_slice(double const *time, long n, double t, long *first) {
  long lo = 0, hi = n - 1;
  while (hi > lo + 1) {
    long const i = (lo + hi) / 2;
    if (time[i] < t) lo = i; else hi = i;
  }
  long const lower = (0 == lo) ? lo : hi;
  lo = lower;
  hi = n - 1;
  while (hi > lo + 1) {
    long const i = (lo + hi) / 2;
    if (time[i] > t) hi = i; else lo = i;
  }
  *first = lower;
  return (int)(((hi == n - 1) ? n : hi) - lower);
}

/* retrieval window and values of quantity iq (0 p, 1 T, 2+g q, 2+ng+w k) */
static double const *quantity(ctl_t const *ctl, atm_t const *atm, int iq, double *zmin, double *zmax) {
  if (iq == 0) { *zmin = ctl->retp_zmin; *zmax = ctl->retp_zmax; return atm->p; }
  if (iq == 1) { *zmin = ctl->rett_zmin; *zmax = ctl->rett_zmax; return atm->t; }
  if (iq < 2 + ctl->ng) { *zmin = ctl->retq_zmin[iq - 2]; *zmax = ctl->retq_zmax[iq - 2]; return atm->q[iq - 2]; }
  int const w = iq - 2 - ctl->ng;
  *zmin = ctl->retk_zmin[w]; *zmax = ctl->retk_zmax[w];
  return atm->k[w];
}

/* State vector of the atmosphere inside the retrieval windows (atm2x, jurassic.c:1491-1513):
 * quantity index iqa (0 p, 1 T, 2+g q, 2+ng+w k) and atmosphere point ipa per element. */
size_t jur_state_vector(ctl_t const *ctl, atm_t const *atm, double *x, int *iqa, int *ipa) {
  size_t n = 0;
  int const nquant = 2 + ctl->ng + ctl->nw;
  for (int iq = 0; iq < nquant; iq++) {
    double zmin, zmax;
    double const *value = quantity(ctl, atm, iq, &zmin, &zmax);
    for (int ip = 0; ip < atm->np; ip++)
      if (atm->z[ip] >= zmin && atm->z[ip] <= zmax) {
        if (x) x[n] = value[ip];
        if (iqa) iqa[n] = iq;
        if (ipa) ipa[n] = ip;
        n++;
      }
  }
  return n;
}

/* The state elements of the points [first, first + len), in the state vector's order (quantity-major, point index
 * inside): global index, quantity and point of each; any output may be NULL.  Returns their number. */
long jur_scene_slice_elements(ctl_t const *ctl, atm_t const *atm, int first, int len, long *cols, int *iqa, int *ipa) {
  long n = 0, base = 0;
  int const nquant = 2 + ctl->ng + ctl->nw;
  for (int iq = 0; iq < nquant; iq++) {
    double zmin, zmax;
    (void)quantity(ctl, atm, iq, &zmin, &zmax);
    for (int ip = 0; ip < atm->np; ip++) {
      if (!(atm->z[ip] >= zmin && atm->z[ip] <= zmax)) continue;
      if (ip >= first && ip < first + len) {
        if (cols) cols[n] = base;
        if (iqa) iqa[n] = iq;
        if (ipa) ipa[n] = ip;
        n++;
      }
      base++;
    }
  }
  return n;
}

long jur_scene_columns(ctl_t const *ctl, atm_t const *atm, int first, int len, long *cols) {
  if (!ctl || !atm || first < 0 || len < 0 || (long)first + len > atm->np) {
    jur_set_error("scene_columns: slice [%d, %d + %d) outside the atmosphere", first, first, len);
    return JUR_EINVAL;
  }
  return jur_scene_slice_elements(ctl, atm, first, len, cols, NULL, NULL);
}

int jur_scene_layout(ctl_t const *ctl, atm_t const *atm, long nr, double const *time, int *first, int *len, long *rowptr) {
  if (!ctl || !atm || nr < 0 || !rowptr || (nr > 0 && (!time || !first || !len))) { jur_set_error("scene_layout: bad arguments"); return JUR_EINVAL; }
  int const np = atm->np;
  if (np < 2 || np > JUR_NP) { jur_set_error("scene_layout: need 2..%d atmospheric points", JUR_NP); return JUR_EINVAL; }
  /* elements of the state at or before every point, over all quantities: the width of a slice is a difference of two */
  long *upto = (long *)calloc((size_t)np + 1, sizeof(long));
  if (!upto) return JUR_ENOMEM;
  int const nquant = 2 + ctl->ng + ctl->nw;
  for (int iq = 0; iq < nquant; iq++) {
    double zmin, zmax;
    (void)quantity(ctl, atm, iq, &zmin, &zmax);
    for (int ip = 0; ip < np; ip++)
      if (atm->z[ip] >= zmin && atm->z[ip] <= zmax) upto[ip + 1]++;
  }
  for (int ip = 0; ip < np; ip++) upto[ip + 1] += upto[ip];
  rowptr[0] = 0;
  for (long r = 0; r < nr; r++) {
    long lo;
    int const n = jur_atm_slice(atm->time, np, time[r], &lo);
    first[r] = (int)lo;
    len[r] = n;
    rowptr[r + 1] = rowptr[r] + (n >= 2 ? upto[lo + n] - upto[lo] : 0);
  }
  free(upto);
  return JUR_OK;
}

long jur_scene_elements(ctl_t const *ctl, atm_t const *atm, int first, int len, long *cols, int *iq, int *ip) {
  if (!ctl || !atm || first < 0 || len < 0 || (long)first + len > atm->np) {
    jur_set_error("scene_elements: slice [%d, %d + %d) outside the atmosphere", first, first, len);
    return JUR_EINVAL;
  }
  return jur_scene_slice_elements(ctl, atm, first, len, cols, iq, ip);
}

/* The distinct slices (first, len) among the rays that have state elements (rp[r + 1] > rp[r]), in the order the rays
 * first meet them: sid[r] is the slice of ray r, -1 for a ray without elements.  Slices with the same first point are
 * chained through `next` from head[first].  *out is malloc'ed (NULL for no slices); returns their number or JUR_ENOMEM. */
long jur_scene_distinct(int np, long nr, int const *first, int const *len, long const *rp, int *sid, jur_scene_slice_t **out) {
  jur_scene_slice_t *sl = NULL;
  long nslice = 0, cap = 0;
  int *head = (int *)malloc(sizeof(int) * (size_t)(np > 0 ? np : 1));
  *out = NULL;
  if (!head) return JUR_ENOMEM;
  for (int i = 0; i < np; i++) head[i] = -1;
  for (long r = 0; r < nr; r++) {
    sid[r] = -1;
    if (rp[r + 1] == rp[r]) continue;
    int q = head[first[r]];
    while (q >= 0 && sl[q].len != len[r]) q = sl[q].next;
    if (q < 0) {
      if (nslice == cap) {
        cap = cap ? 2 * cap : 64;
        jur_scene_slice_t *grown = (jur_scene_slice_t *)realloc(sl, sizeof *sl * (size_t)cap);
        if (!grown) { free(sl); free(head); return JUR_ENOMEM; }
        sl = grown;
      }
      q = (int)nslice++;
      sl[q].first = first[r]; sl[q].len = len[r]; sl[q].next = head[first[r]];
      sl[q].nel = rp[r + 1] - rp[r];
      head[first[r]] = q;
    }
    sid[r] = q;
  }
  free(head);
  *out = sl;
  return nslice;
}

/* The policy of one iteration of jur_retrieve_scene_host (include/jurassic_hip.h).  `x != x` is the NaN test: +inf is a
 * candidate like any other, and never accepted against a finite J by the strict comparison. */
int jur_retrieve_decide(int nlam, long nslice, double tol, double lam_max, double fac_max, double const *J, double const *Jt,
                        double const *lamt, int const *status, double *lam, int *state, int *best, int *accept) {
  if (nlam < 1 || nslice < 0 || (nslice > 0 && (!J || !Jt || !lamt || !status || !lam || !state || !best || !accept))) {
    jur_set_error("jur_retrieve_decide: bad arguments");
    return JUR_EINVAL;
  }
  for (long s = 0; s < nslice; s++) {
    best[s] = accept[s] = -1;
    if (state[s] != JUR_RET_ACTIVE) continue;
    int b = -1;
    for (int l = 0; l < nlam; l++) {
      size_t const at = (size_t)l * (size_t)nslice + (size_t)s;
      if (status[at] != 0 || Jt[at] != Jt[at]) continue;
      if (b < 0 || Jt[at] < Jt[(size_t)b * (size_t)nslice + (size_t)s]) b = l;
    }
    best[s] = b;
    double const jb = b >= 0 ? Jt[(size_t)b * (size_t)nslice + (size_t)s] : 0.;
    accept[s] = (b >= 0 && jb < J[s]) ? 1 : 0;
    if (accept[s]) {
      lam[s] = lamt[(size_t)b * (size_t)nslice + (size_t)s];
      if (J[s] - jb <= tol * J[s]) state[s] = JUR_RET_CONVERGED;
    } else if (lam[s] == lam_max) state[s] = JUR_RET_STALLED;
    else {
      double const grown = lam[s] * fac_max;
      lam[s] = grown < lam_max ? grown : lam_max;
    }
  }
  return JUR_OK;
}

long jur_scene_slices(ctl_t const *ctl, atm_t const *atm, long nr, double const *time, int *sid, int *sfirst, int *slen,
                      long *wptr, long *aptr) {
  if (!ctl || !atm || nr < 0 || (nr > 0 && !time)) { jur_set_error("scene_slices: bad arguments"); return JUR_EINVAL; }
  size_t const NR = (size_t)nr;
  int *first = (int *)malloc(sizeof(int) * (3 * NR + 1)), *len = first ? first + NR : NULL, *own = first ? len + NR : NULL;
  long *rp = (long *)malloc(sizeof(long) * (NR + 1));
  jur_scene_slice_t *sl = NULL;
  long n = JUR_ENOMEM;
  if (!first || !rp) { jur_set_error("scene_slices: out of memory"); goto done; }
  if ((n = jur_scene_layout(ctl, atm, nr, time, first, len, rp))) goto done;
  n = jur_scene_distinct(atm->np, nr, first, len, rp, sid ? sid : own, &sl);
  if (n < 0) { jur_set_error("scene_slices: out of memory"); goto done; }
  if (wptr) wptr[0] = 0;
  if (aptr) aptr[0] = 0;
  for (long q = 0; q < n; q++) {
    if (sfirst) sfirst[q] = sl[q].first;
    if (slen) slen[q] = sl[q].len;
    if (wptr) wptr[q + 1] = wptr[q] + sl[q].nel;
    if (aptr) aptr[q + 1] = aptr[q] + sl[q].nel * sl[q].nel;
  }
done:
  free(first); free(rp); free(sl);
  return n;
}

/* ---- field of view of the scene entries: scans, windows and the effective mask ---------------------------------------- */
typedef struct { double time; long start; } fov_run_t;

static int fov_run_cmp(void const *pa, void const *pb) {
  fov_run_t const *a = (fov_run_t const *)pa, *b = (fov_run_t const *)pb;
  if (a->time < b->time) return -1;
  if (a->time > b->time) return 1;
  return (a->start > b->start) - (a->start < b->start);
}

long jur_scene_fov_live(int nd, long nr, double const *time, double const *rad_in, unsigned char *live) {
  if (nd < 1 || nr < 0 || (nr > 0 && (!time || !rad_in))) { jur_set_error("jur_scene_fov_live: bad arguments"); return JUR_EINVAL; }
  if (nr == 0) return 0;
  /* a time stamp in two separate runs: the runs sorted by time stamp, then by start (NaN equals nothing: a run of one) */
  long nrun = 0;
  for (long r = 0; r < nr; r++) nrun += (r == 0 || !(time[r] == time[r - 1]));
  fov_run_t *run = (fov_run_t *)malloc(sizeof *run * (size_t)nrun);
  if (!run) { jur_set_error("jur_scene_fov_live: out of memory"); return JUR_ENOMEM; }
  long n = 0, again = -1;
  for (long r = 0; r < nr; r++)
    if ((r == 0 || !(time[r] == time[r - 1])) && time[r] == time[r]) { run[n].time = time[r]; run[n].start = r; n++; }
  qsort(run, (size_t)n, sizeof *run, fov_run_cmp);
  for (long i = 1; i < n; i++)
    if (run[i].time == run[i - 1].time && (again < 0 || run[i].start < again)) again = run[i].start;
  free(run);
  if (again >= 0) {
    jur_set_error("jur_scene_fov_live: ray %ld starts a second run of rays with the time stamp %.17g: the rays of a scan must "
                  "follow one another", again, time[again]);
    return JUR_EINVAL;
  }
  long count = 0;
  for (long r = 0; r < nr; r++) {
    long const lo = r - JUR_NFOV > 0 ? r - JUR_NFOV : 0, hi = r + 1 + JUR_NFOV < nr ? r + 1 + JUR_NFOV : nr;
    int nz = 0;
    for (long r2 = lo; r2 < hi; r2++) nz += time[r2] == time[r];
    if (nz < 2) {
      jur_set_error("jur_scene_fov_live: ray %ld is alone in its window: Cannot apply FOV convolution!", r);
      return JUR_EINVAL;
    }
    for (int id = 0; id < nd; id++) {
      int ok = 1;
      for (long r2 = lo; r2 < hi && ok; r2++)
        if (time[r2] == time[r] && !isfinite(rad_in[(size_t)r2 * (size_t)nd + (size_t)id])) ok = 0;
      if (live) live[(size_t)r * (size_t)nd + (size_t)id] = (unsigned char)ok;
      count += ok;
    }
  }
  return count;
}

/* ---- passes of the scene entries: the two cuts and what a looping call reserves for them ----------------------------- */
long jur_scene_passes(long nr, long const *rp, long cap, double const *time, long *pass, long *nmax, long *kmax) {
  if (nr < 0 || cap < 1 || !rp) { jur_set_error("jur_scene_passes: bad arguments"); return JUR_EINVAL; }
  long npass = 0, slots = 0, cols = 0;
  for (long r0 = 0; r0 < nr;) {
    long r1 = r0 + 1;
    while (r1 < nr && (rp[r1 + 1] - rp[r0]) + (r1 + 1 - r0) <= cap) r1++;
    while (time && r1 < nr && time[r1] == time[r1 - 1]) r1++;   /* (a field of view is set: to the end of the scan) */
    long const n = (rp[r1] - rp[r0]) + (r1 - r0);
    if (n > 0x7fffffffL) { jur_set_error("jur_scene_passes: a pass of 2^31 slots"); return JUR_EINVAL; }
    if (n > slots) slots = n;
    if (rp[r1] - rp[r0] > cols) cols = rp[r1] - rp[r0];
    if (pass) pass[npass] = r0;
    npass++;
    r0 = r1;
  }
  if (pass) pass[npass] = nr;
  if (nmax) *nmax = slots;
  if (kmax) *kmax = cols;
  return npass;
}

long jur_trial_passes(long nr, int ntrial, long cap, double const *time, long *pass, long *nmax) {
  if (nr < 0 || ntrial < 1 || cap < 1) { jur_set_error("jur_trial_passes: bad arguments"); return JUR_EINVAL; }
  long per = cap / ntrial, npass = 0, slots = 0;
  if (per < 1) per = 1;
  if (per > 0x7fffffffL / ntrial) per = 0x7fffffffL / ntrial;
  for (long r0 = 0; r0 < nr;) {
    long r1 = r0 + per < nr ? r0 + per : nr;
    while (time && r1 < nr && time[r1] == time[r1 - 1]) r1++;   /* (a field of view is set: to the end of the scan) */
    if ((r1 - r0) * ntrial > 0x7fffffffL) { jur_set_error("jur_trial_passes: a pass of 2^31 slots"); return JUR_EINVAL; }
    if ((r1 - r0) * ntrial > slots) slots = (r1 - r0) * ntrial;
    if (pass) pass[npass] = r0;
    npass++;
    r0 = r1;
  }
  if (pass) pass[npass] = nr;
  if (nmax) *nmax = slots;
  return npass;
}

int jur_scene_pass_reserve(long nr, long const *rp, long cap, int ntrial, double const *time, long *slots, long *cols) {
  if (nr < 0 || cap < 1 || ntrial < 1 || !rp || !slots || !cols) { jur_set_error("jur_scene_pass_reserve: bad arguments"); return JUR_EINVAL; }
  long const all = rp[nr] + nr, tall = nr * ntrial;
  long jb, kb, tb;
  if (time) {
    /* A pass of the rays that remain is cut within the cap (or is one ray beyond it) and then extended to the end of its
     * last scan, of which it already holds a ray: it grows by less than the largest scan.  Scans leave whole (a slice ends
     * with all rays of its time stamp), so the scans that remain are the call's.  Room for the cap and one more scan, of
     * either kind, and never more than all rays together; the first cut is one such cut. */
    long scan_slots = 0, scan_cols = 0, scan_rays = 0;
    for (long r0 = 0, r1; r0 < nr; r0 = r1) {
      for (r1 = r0 + 1; r1 < nr && time[r1] == time[r0]; r1++);
      if ((rp[r1] - rp[r0]) + (r1 - r0) > scan_slots) scan_slots = (rp[r1] - rp[r0]) + (r1 - r0);
      if (rp[r1] - rp[r0] > scan_cols) scan_cols = rp[r1] - rp[r0];
      if (r1 - r0 > scan_rays) scan_rays = r1 - r0;
    }
    jb = cap < all - scan_slots ? cap + scan_slots : all;
    kb = cap < rp[nr] - scan_cols ? cap + scan_cols : rp[nr];
    tb = cap / ntrial + 1 + scan_rays < nr ? (cap / ntrial + 1 + scan_rays) * ntrial : tall;
  } else {
    /* jur_scene_passes extends a pass only while its slots stay within the cap, so a pass of any subset of the rays is
     * within the cap -- and within all rays together -- or is one ray whose width + 1 slots alone exceed the cap; that
     * ray is in the call and went alone in the first cut too.  Hence slots <= max(min(cap, all), widest ray + 1).  A pass
     * within the cap spends one slot per ray on the unperturbed ray, so its block columns are at most cap - 1, and at
     * most all columns together; the one ray beyond the cap has its own width: columns <= max(min(cap - 1, rp[nr]),
     * widest ray).  The greedy cut of a subset can reach these where the first cut does not: rays that it kept apart
     * become neighbours once the rays between them have left.  jur_trial_passes takes max(cap / ntrial, 1) rays per pass,
     * whatever they are, so on fewer rays no pass has more: min(that, nr) rays, as in the first cut. */
    long wide = 0;
    for (long r = 0; r < nr; r++) if (rp[r + 1] - rp[r] > wide) wide = rp[r + 1] - rp[r];
    jb = cap < all ? cap : all;
    if (nr > 0 && wide + 1 > jb) jb = wide + 1;
    kb = cap - 1 < rp[nr] ? cap - 1 : rp[nr];
    if (wide > kb) kb = wide;
    long per = cap / ntrial;
    if (per < 1) per = 1;
    if (per > 0x7fffffffL / ntrial) per = 0x7fffffffL / ntrial;
    tb = (per < nr ? per : nr) * ntrial;
  }
  *slots = jb > tb ? jb : tb;
  *cols = kb;
  return JUR_OK;
}

/* ---- the Jacobian reused between iterations (jur_model_set_kernel_recomp): where the retained blocks lie -------------- */
long jur_scene_recomp_offsets(long nr, long const *rp, int const *sid, int const *then, int const *now, int nd, long *koff) {
  if (nr < 0 || nd < 1 || (nr > 0 && (!rp || !sid || !then || !now || !koff))) { jur_set_error("jur_scene_recomp_offsets: bad arguments"); return JUR_EINVAL; }
  long n = 0, at = 0;                               /* the rays active now, the block columns written before this ray */
  for (long r = 0; r < nr; r++) {
    if (sid[r] < 0) continue;
    int const was = then[sid[r]] == JUR_RET_ACTIVE;
    if (now[sid[r]] == JUR_RET_ACTIVE) {
      if (!was) {
        jur_set_error("jur_scene_recomp_offsets: slice %d of ray %ld is active but was not when the Jacobian was computed", sid[r], r);
        return JUR_EINVAL;
      }
      koff[n++] = at * nd;
    }
    if (was) at += rp[r + 1] - rp[r];
  }
  return n;
}

/* ---- the rays of the slices: their lists, and the rays that remain once slices of a retrieval have ended ------------- */
long jur_scene_rays_by_slice(long nr, long nslice, int const *sid, long *sptr, int *srays) {
  for (long q = 0; q <= nslice; q++) sptr[q] = 0;
  for (long r = 0; r < nr; r++) if (sid[r] >= 0) sptr[sid[r] + 1]++;
  for (long q = 0; q < nslice; q++) sptr[q + 1] += sptr[q];
  for (long r = 0; r < nr; r++) if (sid[r] >= 0) srays[sptr[sid[r]]++] = (int)r;   /* (sptr[q] now ends slice q ...) */
  for (long q = nslice; q > 0; q--) sptr[q] = sptr[q - 1];                          /* ... and starts it again      */
  sptr[0] = 0;
  return sptr[nslice];
}

long jur_scene_gather_active(long nr, long nslice, long const *rp, int const *sid, int const *state, long const *sptr,
                             int const *srays, int *act, int *pos, long *rpc, long *sptrc, int *sraysc) {
  long n = 0, nl = 0;
  rpc[0] = 0;
  for (long r = 0; r < nr; r++) {
    pos[r] = -1;
    if (sid[r] < 0 || state[sid[r]] != JUR_RET_ACTIVE) continue;
    act[n] = (int)r; pos[r] = (int)n;
    rpc[n + 1] = rpc[n] + (rp[r + 1] - rp[r]);
    n++;
  }
  for (long q = 0; q < nslice; q++) {
    sptrc[q] = nl;
    if (state[q] == JUR_RET_ACTIVE)
      for (long i = sptr[q]; i < sptr[q + 1]; i++) sraysc[nl++] = pos[srays[i]];
  }
  sptrc[nslice] = nl;
  return n;
}

/* ---- posterior diagnostics (jur_diagnose_slices_host, jur_diagnose_scene_host): the host arithmetic ------------------ */
int jur_diag_check_out(char const *who, jur_diag_out_t const *out) {
  if (!out) { jur_set_error("%s: null argument (out)", who); return JUR_EINVAL; }
  char const *const missing = !out->sigma ? "sigma" : !out->sigma_noise ? "sigma_noise" : !out->sigma_smooth ? "sigma_smooth"
                            : !out->avk_diag ? "avk_diag" : !out->dofs ? "dofs" : !out->status ? "status" : NULL;
  if (missing) { jur_set_error("%s: null argument (%s)", who, missing); return JUR_EINVAL; }
  return JUR_OK;
}

int jur_diag_check_wptr(char const *who, long nslice, long const *wptr) {
  if (nslice < 0 || (nslice > 0 && !wptr)) { jur_set_error("%s: bad arguments", who); return JUR_EINVAL; }
  for (long q = 0; q < nslice; q++) {
    long const w = wptr[q + 1] - wptr[q];
    if (wptr[0] != 0 || w < 0 || w > 0x7fffffffL) {
      jur_set_error("%s: wptr is not an ascending running sum of widths from 0 (slice %ld)", who, q);
      return JUR_EINVAL;
    }
  }
  return JUR_OK;
}

int jur_diag_check_prior(char const *who, long nslice, long const *wptr, double const *prior_ivar) {
  if (!prior_ivar) return JUR_OK;
  for (long q = 0; q < nslice; q++)
    for (long e = wptr[q]; e < wptr[q + 1]; e++) {
      double const r = prior_ivar[e];
      if (!(r >= 0) || r > 1.7976931348623157e308) {
        jur_set_error("%s: prior_ivar of slice %ld, element %ld is %g: negative or not finite", who, q, e - wptr[q], r);
        return JUR_EINVAL;
      }
    }
  return JUR_OK;
}

/* ---- full a-priori precision (jur_model_set_prior_precision, jur_prior_corr_host): the host checks ------------------- */
/* R_s at R + aptr[s], [w_s][w_s]: the diagonal and the lower triangle (what is read) finite, R_ii >= 0 */
int jur_prior_check_R(char const *who, long nslice, long const *wptr, double const *R) {
  int const rc = jur_diag_check_wptr(who, nslice, wptr);
  if (rc) return rc;
  if (nslice > 0 && wptr[nslice] > 0 && !R) { jur_set_error("%s: null argument (R)", who); return JUR_EINVAL; }
  size_t at = 0;
  for (long q = 0; q < nslice; q++) {
    size_t const w = (size_t)(wptr[q + 1] - wptr[q]);
    for (size_t i = 0; i < w; i++) {
      for (size_t j = 0; j <= i; j++) {
        double const v = R[at + i * w + j];
        if (!(v - v == 0)) {
          jur_set_error("%s: R of slice %ld, element (%zu, %zu) is %g: not finite", who, q, i, j, v);
          return JUR_EINVAL;
        }
      }
      if (R[at + i * w + i] < 0) {
        jur_set_error("%s: R of slice %ld, element (%zu, %zu) is %g: a negative diagonal", who, q, i, i, R[at + i * w + i]);
        return JUR_EINVAL;
      }
    }
    at += w * w;
  }
  return JUR_OK;
}

/* the layout of a call against the one the precision was set with (set_wptr: [set_nslice + 1]) */
int jur_prior_check_layout(char const *who, long set_nslice, long const *set_wptr, long nslice, long const *wptr) {
  if (set_nslice != nslice) {
    jur_set_error("%s: the call has %ld slices, the prior precision of the model was set for %ld", who, nslice, set_nslice);
    return JUR_EINVAL;
  }
  for (long q = 0; q < nslice; q++) {
    long const w = wptr[q + 1] - wptr[q], ws = set_wptr[q + 1] - set_wptr[q];
    if (w != ws) {
      jur_set_error("%s: slice %ld of the call has %ld elements, the prior precision of the model was set for %ld", who, q, w, ws);
      return JUR_EINVAL;
    }
  }
  return JUR_OK;
}

int jur_prior_check_corr(char const *who, long nslice, long const *wptr, int const *iq, double const *z, double const *sigma,
                         int nq, double const *cz) {
  int const rc = jur_diag_check_wptr(who, nslice, wptr);
  if (rc) return rc;
  if (nq < 0 || (nq > 0 && !cz)) { jur_set_error("%s: bad arguments (nq, cz)", who); return JUR_EINVAL; }
  for (int q = 0; q < nq; q++)
    if (!(cz[q] >= 0) || !(cz[q] - cz[q] == 0)) {
      jur_set_error("%s: cz of quantity %d is %g: negative or not finite", who, q, cz[q]);
      return JUR_EINVAL;
    }
  if (nslice > 0 && wptr[nslice] > 0 && (!iq || !z || !sigma)) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  for (long q = 0; q < nslice; q++)
    for (long e = wptr[q]; e < wptr[q + 1]; e++) {
      if (iq[e] < 0 || iq[e] >= nq) {
        jur_set_error("%s: iq of slice %ld, element %ld is %d: outside 0..%d", who, q, e - wptr[q], iq[e], nq - 1);
        return JUR_EINVAL;
      }
      if (!(sigma[e] > 0) || !(sigma[e] - sigma[e] == 0)) {
        jur_set_error("%s: sigma of slice %ld, element %ld is %g: not positive or not finite", who, q, e - wptr[q], sigma[e]);
        return JUR_EINVAL;
      }
      if (!(z[e] - z[e] == 0)) {
        jur_set_error("%s: z of slice %ld, element %ld is %g: not finite", who, q, e - wptr[q], z[e]);
        return JUR_EINVAL;
      }
    }
  return JUR_OK;
}

/* Block b of the inverse is columns [c0, c0 + 16) of system s: imap[2 b] = s, imap[2 b + 1] = c0, systems ascending and
 * columns ascending within a system.  Tile t of the product is rows [i0, i0 + 64) x columns [j0, j0 + 64) of system s:
 * tmap[3 t] = s, then i0, j0, row-major within a system.  A system of width 0 has neither. */
long jur_diag_maps(long nslice, long const *wptr, int *imap, int *tmap, long *ntile) {
  long ninv = 0, nt = 0;
  for (long q = 0; q < nslice; q++) {
    long const w = wptr[q + 1] - wptr[q];
    for (long c0 = 0; c0 < w; c0 += JUR_DIAG_NB, ninv++)
      if (imap) { imap[2 * ninv] = (int)q; imap[2 * ninv + 1] = (int)c0; }
    for (long i0 = 0; i0 < w; i0 += JUR_DIAG_TILE)
      for (long j0 = 0; j0 < w; j0 += JUR_DIAG_TILE, nt++)
        if (tmap) { tmap[3 * nt] = (int)q; tmap[3 * nt + 1] = (int)i0; tmap[3 * nt + 2] = (int)j0; }
  }
  if (ntile) *ntile = nt;
  return ninv;
}

/* ---- gain matrix and error budget (jur_gain_slices_host, jur_gain_scene_host): the host arithmetic ------------------- */
int jur_gain_check_args(char const *who, jur_gain_in_t const *in, jur_gain_out_t const *out) {
  if (!in || !out) { jur_set_error("%s: null argument (%s)", who, !in ? "in" : "out"); return JUR_EINVAL; }
  if (in->ncomp < 0 || in->ncomp > JUR_GAIN_MAXCOMP) {
    jur_set_error("%s: ncomp = %d: 0 to %d components per call", who, in->ncomp, JUR_GAIN_MAXCOMP);
    return JUR_EINVAL;
  }
  if (in->ncomp > 0 && !out->sigma_comp) { jur_set_error("%s: null argument (sigma_comp) with ncomp = %d", who, in->ncomp); return JUR_EINVAL; }
  if (in->ncomp > 0 && !in->var) { jur_set_error("%s: null argument (var) with ncomp = %d", who, in->ncomp); return JUR_EINVAL; }
  return JUR_OK;
}

int jur_gain_check_layout(char const *who, long nslice, long const *wptr, long nr, long const *rowptr, int const *sid) {
  if (rowptr[0] != 0) { jur_set_error("%s: rowptr does not start at 0", who); return JUR_EINVAL; }
  for (long r = 0; r < nr; r++) {
    if (sid[r] < -1 || sid[r] >= nslice) {
      jur_set_error("%s: sid of ray %ld is %d: outside -1..%ld", who, r, sid[r], nslice - 1);
      return JUR_EINVAL;
    }
    long const w = sid[r] < 0 ? 0 : wptr[sid[r] + 1] - wptr[sid[r]];
    if (rowptr[r + 1] - rowptr[r] != w) {
      jur_set_error("%s: the block of ray %ld has %ld columns, its slice %d has %ld elements", who, r, rowptr[r + 1] - rowptr[r], sid[r], w);
      return JUR_EINVAL;
    }
  }
  return JUR_OK;
}

int jur_gain_check_var(char const *who, int ncomp, long nr, int nd, double const *var, unsigned char const *live) {
  size_t const nrd = (size_t)nr * (size_t)nd;
  for (int c = 0; c < ncomp; c++)
    for (long r = 0; r < nr; r++)
      for (int id = 0; id < nd; id++) {
        size_t const at = (size_t)r * (size_t)nd + (size_t)id;
        if (!live[at]) continue;
        double const v = var[(size_t)c * nrd + at];
        if (!(v >= 0) || !(v - v == 0)) {
          jur_set_error("%s: the variance of component %d, ray %ld, channel %d is %g: negative or not finite", who, c, r, id, v);
          return JUR_EINVAL;
        }
      }
  return JUR_OK;
}

long jur_gain_maps(long nslice, long const *wptr, long const *sptr, int nd, int *gmap) {
  long nt = 0;
  for (long q = 0; q < nslice; q++) {
    long const w = wptr[q + 1] - wptr[q], M = (sptr[q + 1] - sptr[q]) * nd;
    if (M > 0x7fffffffL) return -1;
    for (long m0 = 0; m0 < M; m0 += JUR_GAIN_TILE)
      for (long i0 = 0; i0 < w; i0 += JUR_GAIN_TILE, nt++)
        if (gmap) { gmap[3 * nt] = (int)q; gmap[3 * nt + 1] = (int)m0; gmap[3 * nt + 2] = (int)i0; }
  }
  return nt;
}

/* upstream's set_cov_meas: the two variances of every measurement and the weight under their sum */
int jur_error_components(int nd, long nr, double const *y, double const *err_noise, double const *err_formod, double *var,
                         double *weight) {
  char const *const who = "jur_error_components";
  if (nd < 0 || nr < 0) { jur_set_error("%s: bad arguments", who); return JUR_EINVAL; }
  if (nd > 0 && (!err_noise || !err_formod)) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  for (int id = 0; id < nd; id++) {
    if (!(err_noise[id] >= 0) || !(err_noise[id] - err_noise[id] == 0)) {
      jur_set_error("%s: err_noise of channel %d is %g: negative or not finite", who, id, err_noise[id]);
      return JUR_EINVAL;
    }
    if (!(err_formod[id] >= 0) || !(err_formod[id] - err_formod[id] == 0)) {
      jur_set_error("%s: err_formod of channel %d is %g: negative or not finite", who, id, err_formod[id]);
      return JUR_EINVAL;
    }
  }
  size_t const nrd = (size_t)nr * (size_t)nd;
  if (nrd == 0) return JUR_OK;
  if (!y || !var || !weight) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  for (long r = 0; r < nr; r++)
    for (int id = 0; id < nd; id++) {
      size_t const at = (size_t)r * (size_t)nd + (size_t)id;
      double const vn = err_noise[id] * err_noise[id], f = err_formod[id] / 100 * y[at], vf = f * f, sum = vn + vf;
      int const ok = sum > 0 && sum - sum == 0;
      var[at] = ok ? vn : 0.;
      var[nrd + at] = ok ? vf : 0.;
      weight[at] = ok ? 1 / sum : 0.;
    }
  return JUR_OK;
}

/* ---- parameter errors (jur_param_slices_host): the host arithmetic ---------------------------------------------------- */
int jur_param_check_args(char const *who, jur_param_in_t const *in, jur_param_out_t const *out) {
  if (!in || !out) { jur_set_error("%s: null argument (%s)", who, !in ? "in" : "out"); return JUR_EINVAL; }
  if (in->nvar < 0 || in->ncov < 0 || (long)in->nvar + in->ncov > JUR_PARAM_MAXCOMP) {
    jur_set_error("%s: nvar = %d, ncov = %d: 0 to %d components per call", who, in->nvar, in->ncov, JUR_PARAM_MAXCOMP);
    return JUR_EINVAL;
  }
  if (in->nvar + in->ncov > 0 && !out->sigma_param) {
    jur_set_error("%s: null argument (sigma_param) with nvar + ncov = %d", who, in->nvar + in->ncov);
    return JUR_EINVAL;
  }
  return JUR_OK;
}

/* The width wb_s of a slice is that of its rays in rowptr_b, 0 without rays; the ray that fixed it is named with the one
 * that disagrees. */
long jur_param_layout_as(char const *who, long nslice, long const *wptr, long nr, long const *rowptr, long const *rowptr_b,
                         int const *sid, long *bwptr, long *cptr, long *bbptr) {
  if (nslice < 0 || nr < 0) { jur_set_error("%s: bad arguments", who); return JUR_EINVAL; }
  if ((nslice > 0 && !wptr) || !rowptr || !rowptr_b || (nr > 0 && !sid)) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  int rc = jur_diag_check_wptr(who, nslice, wptr);
  if (rc) return rc;
  if ((rc = jur_gain_check_layout(who, nslice, wptr, nr, rowptr, sid))) return rc;
  if (rowptr_b[0] != 0) { jur_set_error("%s: rowptr_b does not start at 0", who); return JUR_EINVAL; }
  size_t const NS = (size_t)nslice;
  long *bw = (long *)malloc(sizeof(long) * 2 * (NS ? NS : 1)), *by = bw ? bw + NS : NULL;   /* the width of a slice, the ray that fixed it */
  if (!bw) { jur_set_error("%s: out of memory", who); return JUR_ENOMEM; }
  long total = JUR_EINVAL;
  for (long q = 0; q < nslice; q++) { bw[q] = 0; by[q] = -1; }
  for (long r = 0; r < nr; r++) {
    long const wb = rowptr_b[r + 1] - rowptr_b[r];
    if (wb < 0 || wb > 0x7fffffffL) { jur_set_error("%s: rowptr_b is not ascending at ray %ld", who, r); goto done; }
    int const q = sid[r];
    if (q < 0) continue;
    if (by[q] < 0) { by[q] = r; bw[q] = wb; }
    else if (bw[q] != wb) {
      jur_set_error("%s: rays %ld and %ld of slice %d have %ld and %ld columns in rowptr_b", who, by[q], r, q, bw[q], wb);
      goto done;
    }
  }
  long nbw = 0, nc = 0, nbb = 0;
  for (long q = 0; q <= nslice; q++) {
    if (bwptr) bwptr[q] = nbw;
    if (cptr) cptr[q] = nc;
    if (bbptr) bbptr[q] = nbb;
    if (q == nslice) break;
    nbw += bw[q]; nc += (wptr[q + 1] - wptr[q]) * bw[q]; nbb += bw[q] * bw[q];
  }
  total = nc;
done:
  free(bw);
  return total;
}

long jur_param_layout(long nslice, long const *wptr, long nr, long const *rowptr, long const *rowptr_b, int const *sid,
                      long *bwptr, long *cptr, long *bbptr) {
  return jur_param_layout_as("jur_param_layout", nslice, wptr, nr, rowptr, rowptr_b, sid, bwptr, cptr, bbptr);
}

void jur_param_abi_sizes(size_t out[2]) { out[0] = sizeof(jur_param_in_t); out[1] = sizeof(jur_param_out_t); }

/* bw: the running sum the layout made from rowptr_b */
int jur_param_check_bwptr(char const *who, long nslice, long const *bwptr, long const *bw) {
  for (long q = 0; q < nslice; q++) {
    long const wb = bwptr[q + 1] - bwptr[q];
    if (bwptr[0] != 0 || wb < 0 || wb > 0x7fffffffL) {
      jur_set_error("%s: bwptr is not an ascending running sum of widths from 0 (slice %ld)", who, q);
      return JUR_EINVAL;
    }
    if (wb != bw[q + 1] - bw[q]) {
      jur_set_error("%s: bwptr gives slice %ld %ld columns, its rays have %ld in rowptr_b", who, q, wb, bw[q + 1] - bw[q]);
      return JUR_EINVAL;
    }
  }
  return JUR_OK;
}

int jur_param_check_values(char const *who, long nslice, long const *bwptr, long const *bbptr, jur_param_in_t const *in) {
  size_t const nbw = (size_t)bwptr[nslice], nbb = (size_t)bbptr[nslice];
  if ((in->nvar > 0 && nbw > 0 && !in->var) || (in->ncov > 0 && nbb > 0 && !in->cov)) {
    jur_set_error("%s: null argument (%s)", who, (in->nvar > 0 && nbw > 0 && !in->var) ? "var" : "cov");
    return JUR_EINVAL;
  }
  for (int c = 0; c < in->nvar; c++)
    for (long q = 0; q < nslice; q++)
      for (long j = bwptr[q]; j < bwptr[q + 1]; j++) {
        double const v = in->var[(size_t)c * nbw + (size_t)j];
        if (!(v >= 0) || !(v - v == 0)) {
          jur_set_error("%s: the variance of component %d, slice %ld, element %ld is %g: negative or not finite", who, c, q, j - bwptr[q], v);
          return JUR_EINVAL;
        }
      }
  for (int c = 0; c < in->ncov; c++)
    for (long q = 0; q < nslice; q++) {
      long const wb = bwptr[q + 1] - bwptr[q];
      double const *const sg = in->cov + (size_t)c * nbb + (size_t)bbptr[q];
      for (long j = 0; j < wb; j++)
        for (long l = 0; l <= j; l++) {
          double const v = sg[j * wb + l];
          if (!(v - v == 0)) {
            jur_set_error("%s: cov of component %d, slice %ld, element (%ld, %ld) is %g: not finite", who, in->nvar + c, q, j, l, v);
            return JUR_EINVAL;
          }
          if (l == j && !(v >= 0)) {
            jur_set_error("%s: the diagonal of cov of component %d, slice %ld, element %ld is %g: negative", who, in->nvar + c, q, j, v);
            return JUR_EINVAL;
          }
        }
    }
  return JUR_OK;
}

long jur_param_maps(long nslice, long const *wptr, long const *bwptr, int *cmap) {
  long nt = 0;
  for (long q = 0; q < nslice; q++) {
    long const w = wptr[q + 1] - wptr[q], wb = bwptr[q + 1] - bwptr[q];
    for (long i0 = 0; i0 < w; i0 += JUR_PARAM_TILE)
      for (long j0 = 0; j0 < wb; j0 += JUR_PARAM_TILE, nt++)
        if (cmap) { cmap[3 * nt] = (int)q; cmap[3 * nt + 1] = (int)i0; cmap[3 * nt + 2] = (int)j0; }
  }
  return nt;
}

/* ---- parameter errors of a scene in one call (jur_param_scene_host): the tiles of a pass ----------------------------- */
void jur_param_scene_abi_sizes(size_t out[2]) { out[0] = sizeof(jur_param_scene_in_t); out[1] = sizeof(jur_param_scene_out_t); }

/* the first position in [a, b) of the ascending list whose ray is >= r */
static long rays_lower_bound(int const *srays, long a, long b, long r) {
  while (a < b) {
    long const mid = a + (b - a) / 2;
    if (srays[mid] < r) a = mid + 1; else b = mid;
  }
  return a;
}

void jur_param_pass_range(long const *sptr, int const *srays, long s, long r0, long r1, long *lo, long *hi) {
  *lo = rays_lower_bound(srays, sptr[s], sptr[s + 1], r0);
  *hi = rays_lower_bound(srays, *lo, sptr[s + 1], r1);
}

long jur_param_pass_maps(long const *wptr, long const *bwptr, long const *sptr, int const *srays, int const *sid, long r0, long r1,
                         long *mark, int *pmap) {
  long nt = 0;
  for (long r = r0; r < r1; r++) {
    long const q = sid[r];
    if (q < 0 || mark[q] == r0 + 1) continue;
    mark[q] = r0 + 1;
    long const w = wptr[q + 1] - wptr[q], wb = bwptr[q + 1] - bwptr[q];
    long lo, hi;
    jur_param_pass_range(sptr, srays, q, r0, r1, &lo, &hi);
    for (long i0 = 0; i0 < w; i0 += JUR_PARAM_TILE)
      for (long j0 = 0; j0 < wb; j0 += JUR_PARAM_TILE, nt++) {
        int *const t = pmap + 5 * nt;
        t[0] = (int)q; t[1] = (int)i0; t[2] = (int)j0; t[3] = (int)lo; t[4] = (int)hi;
      }
  }
  return nt;
}

int jur_avk_summary(ctl_t const *ctl, atm_t const *atm, int first, int len, double const *avk, double *dofs_q, double *area,
                    double *resolution) {
  if (!ctl || !atm || first < 0 || len < 0 || (long)first + len > atm->np) {
    jur_set_error("jur_avk_summary: slice [%d, %d + %d) outside the atmosphere", first, first, len);
    return JUR_EINVAL;
  }
  if (!dofs_q) { jur_set_error("jur_avk_summary: null argument (dofs_q)"); return JUR_EINVAL; }
  int const nquant = 2 + ctl->ng + ctl->nw;
  for (int q = 0; q < nquant; q++) dofs_q[q] = 0.;
  long const w = jur_scene_slice_elements(ctl, atm, first, len, NULL, NULL, NULL);
  if (w == 0) return JUR_OK;
  if (!avk || !area || !resolution) { jur_set_error("jur_avk_summary: null argument"); return JUR_EINVAL; }
  int *iq = (int *)malloc(sizeof(int) * 2 * (size_t)w), *ip = iq ? iq + w : NULL;
  if (!iq) { jur_set_error("jur_avk_summary: out of memory"); return JUR_ENOMEM; }
  (void)jur_scene_slice_elements(ctl, atm, first, len, NULL, iq, ip);
  /* the elements of one quantity are contiguous, their points ascending */
  for (long i = 0; i < w; i++) {
    double const d = avk[(size_t)i * (size_t)w + (size_t)i];
    dofs_q[iq[i]] += d;
    double sum = 0.;
    for (long j = 0; j < w; j++)
      if (iq[j] == iq[i]) sum += avk[(size_t)i * (size_t)w + (size_t)j];
    area[i] = sum;
    int const below = i > 0 && iq[i - 1] == iq[i], above = i + 1 < w && iq[i + 1] == iq[i];
    double dz = 0.;
    if (below && above) dz = fabs(atm->z[ip[i + 1]] - atm->z[ip[i - 1]]) / 2;
    else if (above) dz = fabs(atm->z[ip[i + 1]] - atm->z[ip[i]]);
    else if (below) dz = fabs(atm->z[ip[i]] - atm->z[ip[i - 1]]);
    resolution[i] = d > 0 ? dz / d : INFINITY;
  }
  free(iq);
  return JUR_OK;
}

/* ---- hydrostatic balance: one profile (formod()'s adjustment) and the segments of a scene ---------------------------- */
/* (jr_common.h:212-217) */
static double gravity(double z, double lat) {
  double const deg2rad = M_PI / 180., x = sin(lat * deg2rad), y = sin(2 * lat * deg2rad);
  return 9.780318 * (1. + 0.0053024 * x * x - 5.8e-6 * y * y) - 3.086e-3 * z;
}

static double lin(double x0, double y0, double x1, double y1, double x) { return y0 + (x - x0) * (y1 - y0) / (x1 - x0); }

static void layer_pressure(double const *z, double const *t, double const *qh2o, double *p, double lat, int from, int to) {
  /* integrates the hydrostatic equation across one layer with 20 sub-points */
  int const npts = 20;
  double const mmair = 28.96456e-3, mmh2o = 18.0153e-3;
  double mean = 0., e = 0.;
  for (int i = 0; i < npts; i++) {
    double const zz = lin(0.0, z[from], npts - 1.0, z[to], (double)i);
    double const grav = gravity(zz, lat);
    if (qh2o) e = lin(0.0, qh2o[from], npts - 1.0, qh2o[to], (double)i);
    double const temp = lin(0.0, t[from], npts - 1.0, t[to], (double)i);
    mean += (e * mmh2o + (1 - e) * mmair) * grav / (JUR_MOLAR_GAS * temp * npts);
  }
  p[to] = p[from] * exp(-1000 * mean * (z[to] - z[from]));
}

/* hydrostatic_1d_h2o (jr_common.h:713-761) on the n points of one profile: the pressures above and below the point
 * nearest to hydz (the first of several) follow from it; qh2o == NULL: dry air */
void jur_hydrostatic_profile(double hydz, int n, double const *z, double const *lat, double const *t, double const *qh2o,
                             double *p) {
  double dzmin = 1e99;
  int ipref = 0;
  for (int ip = 0; ip < n; ip++) {
    double const dz = fabs(z[ip] - hydz);
    if (dz < dzmin) { dzmin = dz; ipref = ip; }
  }
  for (int ip = ipref + 1; ip < n; ip++) layer_pressure(z, t, qh2o, p, lat[ipref], ip - 1, ip);
  for (int ip = ipref - 1; ip >= 0; ip--) layer_pressure(z, t, qh2o, p, lat[ipref], ip + 1, ip);
}

/* the segments of a balance: inside 0..np, and no point in two segments of two points or more */
int jur_scene_hydro_check(char const *who, int np, long nseg, int const *sfirst, int const *slen) {
  if (np < 0 || nseg < 0 || (nseg > 0 && (!sfirst || !slen))) { jur_set_error("%s: bad arguments", who); return JUR_EINVAL; }
  for (long q = 0; q < nseg; q++)
    if (sfirst[q] < 0 || slen[q] < 0 || (long)sfirst[q] + slen[q] > np) {
      jur_set_error("%s: segment %ld, [%d, %d + %d), lies outside the %d points of the atmosphere", who, q, sfirst[q], sfirst[q],
                    slen[q], np);
      return JUR_EINVAL;
    }
  long *owner = (long *)malloc(sizeof(long) * (size_t)(np > 0 ? np : 1));
  if (!owner) { jur_set_error("%s: out of memory", who); return JUR_ENOMEM; }
  for (int i = 0; i < np; i++) owner[i] = -1;
  int rc = JUR_OK;
  for (long q = 0; q < nseg && !rc; q++) {
    if (slen[q] < 2) continue;
    for (int i = sfirst[q]; i < sfirst[q] + slen[q]; i++) {
      if (owner[i] >= 0) {
        long const o = owner[i];
        jur_set_error("%s: the segments %ld, [%d, %d), and %ld, [%d, %d), share point %d of the atmosphere: a hydrostatic balance "
                      "of each would move the other's pressures", who, o, sfirst[o], sfirst[o] + slen[o], q, sfirst[q],
                      sfirst[q] + slen[q], i);
        rc = JUR_EINVAL;
        break;
      }
      owner[i] = q;
    }
  }
  free(owner);
  return rc;
}

int jur_scene_hydrostatic(ctl_t const *ctl, double hydz, atm_t const *in, long nseg, int const *sfirst, int const *slen,
                          atm_t *out) {
  char const *const who = "jur_scene_hydrostatic";
  if (!ctl || !in || !out) { jur_set_error("%s: null argument", who); return JUR_EINVAL; }
  if (!(hydz >= 0) || !(hydz - hydz == 0)) { jur_set_error("%s: hydz is %g: negative or not finite", who, hydz); return JUR_EINVAL; }
  if (in->np < 0 || in->np > JUR_NP) { jur_set_error("%s: np = %d outside 0..%d", who, in->np, JUR_NP); return JUR_EINVAL; }
  int const rc = jur_scene_hydro_check(who, in->np, nseg, sfirst, slen);
  if (rc) return rc;
  /* the emitter jur_model_set_atm's step reads */
  int ig = -1;
  if (ctl->ctm_h2o)
    for (int g = 0; g < ctl->ng && ig < 0; g++)
      if (0 == strcasecmp(ctl->emitter[g], "H2O")) ig = g;
  if (out != in) memmove(out->p, in->p, sizeof(double) * (size_t)in->np);
  for (long q = 0; q < nseg; q++) {
    if (slen[q] < 2) continue;
    int const a = sfirst[q];
    jur_hydrostatic_profile(hydz, slen[q], in->z + a, in->lat + a, in->t + a, ig >= 0 ? in->q[ig] + a : NULL, out->p + a);
  }
  return JUR_OK;
}

/* the distinct slices of two points or more among (first[r], len[r]), in the order the rays first meet them */
long jur_scene_ray_slices_of(int np, long nr, int const *first, int const *len, int *sfirst, int *slen) {
  long *rp = (long *)malloc(sizeof(long) * ((size_t)nr + 1));
  int *sid = (int *)malloc(sizeof(int) * (size_t)(nr > 0 ? nr : 1));
  jur_scene_slice_t *sl = NULL;
  long n = JUR_ENOMEM;
  if (rp && sid) {
    rp[0] = 0;
    for (long r = 0; r < nr; r++) rp[r + 1] = rp[r] + (len[r] >= 2);   /* (jur_scene_distinct skips rays of width 0) */
    n = jur_scene_distinct(np, nr, first, len, rp, sid, &sl);
    for (long q = 0; q < n; q++) {
      if (sfirst) sfirst[q] = sl[q].first;
      if (slen) slen[q] = sl[q].len;
    }
  }
  free(rp); free(sid); free(sl);
  return n;
}

long *jur_scene_hydro_segments(size_t nh, long nr, long nrs, int const *hyf, long ncopy, long const *off, int const *prow,
                               int row_h2o, long tncopy, long const *toff, long *nhc, long *ntc) {
  long *const at = (long *)malloc((sizeof(long) + sizeof(int)) * (nh ? nh : 1));
  *nhc = *ntc = 0;
  if (!at) return NULL;
  int *const len = (int *)(at + nh);
  long n = 0;
  for (long q = 0; q < nrs; q++, n++) { at[n] = hyf[q]; len[n] = hyf[nr + q]; }
  for (long j = 1; j < ncopy; j++)
    if (prow[j] == 4 || prow[j] == 5 || prow[j] == row_h2o) { at[n] = off[j]; len[n] = (int)(off[j + 1] - off[j]); n++; ++*nhc; }
  for (long j = 1; j < tncopy; j++, n++, ++*ntc) { at[n] = toff[j]; len[n] = (int)(toff[j + 1] - toff[j]); }
  return at;
}

long jur_scene_default_cap(long budget, long used, size_t slot_bytes) {
  long const cap = (budget - used) / 16 / (long)slot_bytes;
  return cap < 4096 ? 4096 : cap;
}

long jur_scene_ray_slices(ctl_t const *ctl, atm_t const *atm, long nr, double const *time, int *sfirst, int *slen) {
  if (!ctl || !atm || nr < 0 || (nr > 0 && !time)) { jur_set_error("scene_ray_slices: bad arguments"); return JUR_EINVAL; }
  int const np = atm->np;
  if (np < 2 || np > JUR_NP) { jur_set_error("scene_ray_slices: need 2..%d atmospheric points", JUR_NP); return JUR_EINVAL; }
  size_t const NR = (size_t)(nr > 0 ? nr : 1);
  int *first = (int *)malloc(sizeof(int) * 2 * NR), *len = first ? first + NR : NULL;
  if (!first) { jur_set_error("scene_ray_slices: out of memory"); return JUR_ENOMEM; }
  for (long r = 0; r < nr; r++) {
    long lo;
    len[r] = jur_atm_slice(atm->time, np, time[r], &lo);
    first[r] = (int)lo;
  }
  long const n = jur_scene_ray_slices_of(np, nr, first, len, sfirst, slen);
  if (n < 0) jur_set_error("scene_ray_slices: out of memory");
  free(first);
  return n;
}

/* ---- the box on the state (jur_model_set_state_bounds) ------------------------------------------------------------------ */
double jur_state_bound(double x, double lo, double hi) {
  double c;
  JUR_STATE_BOUND(c, x, lo, hi);
  return c;
}

/* ---- untraceable rays in the scene retrieval (jur_model_set_scene_overflow) --------------------------------------------- */
int jur_np_overflows(int np) { return JUR_NP_OVERFLOWS(np); }

/* the workgroups (of 256 lanes) the fold runs with over `lanes` flags, and with them its partial counts */
long jur_scene_overflow_parts(long lanes) {
  long const g = (lanes + 255) / 256;
  return g < 1 ? 1 : g > JUR_OVERFLOW_PARTS ? JUR_OVERFLOW_PARTS : g;
}

/* the name of quantity iq for a message: p, T, q[g] (with the emitter where the control is at hand), k[w] */
static char const *quantity_name(int ng, int iq, char buf[32]) {
  if (iq == 0) return "p";
  if (iq == 1) return "T";
  if (iq < 2 + ng) snprintf(buf, 32, "q[%d]", iq - 2);
  else snprintf(buf, 32, "k[%d]", iq - 2 - ng);
  return buf;
}

int jur_state_bounds_check(char const *who, int ng, int nw, int nq, double const *lo, double const *hi) {
  char name[32];
  if (nq != 2 + ng + nw) {
    jur_set_error("%s: nq = %d, the model has %d quantities (p, T, %d q, %d k)", who, nq, 2 + ng + nw, ng, nw);
    return JUR_EINVAL;
  }
  for (int iq = 0; iq < nq; iq++) {
    if (lo[iq] != lo[iq] || hi[iq] != hi[iq]) {
      jur_set_error("%s: the %s bound of quantity %d (%s) is NaN (-inf or +inf leaves a side open)", who, lo[iq] != lo[iq] ? "lower" : "upper",
                    iq, quantity_name(ng, iq, name));
      return JUR_EINVAL;
    }
    if (lo[iq] > hi[iq]) {
      jur_set_error("%s: quantity %d (%s): lo = %g > hi = %g", who, iq, quantity_name(ng, iq, name), lo[iq], hi[iq]);
      return JUR_EINVAL;
    }
  }
  return JUR_OK;
}

void jur_state_bounds_expand(double const *lo, double const *hi, long n, int const *erow, double *elo, double *ehi) {
  for (long e = 0; e < n; e++) { elo[e] = lo[erow[e] - 4]; ehi[e] = hi[erow[e] - 4]; }
}

int jur_state_bounds_upstream(ctl_t const *ctl, double *lo, double *hi) {
  if (!ctl || ctl->ng < 0 || ctl->ng > JUR_NG || ctl->nw < 0 || ctl->nw > JUR_NW) { jur_set_error("jur_state_bounds_upstream: bad arguments"); return JUR_EINVAL; }
  int const nq = 2 + ctl->ng + ctl->nw;
  for (int iq = 0; iq < nq; iq++) {
    double const l = iq == 0 ? 5e-7 : iq == 1 ? 100. : 0., h = iq == 0 ? 5e4 : iq == 1 ? 400. : iq < 2 + ctl->ng ? 1. : INFINITY;
    if (lo) lo[iq] = l;
    if (hi) hi[iq] = h;
  }
  return nq;
}

long jur_state_on_bounds(int nq, double const *lo, double const *hi, long n, int const *iq, double const *x, signed char *side) {
  char const *const who = "jur_state_on_bounds";
  if (nq < 0 || n < 0 || (nq > 0 && (!lo || !hi)) || (n > 0 && (!iq || !x))) { jur_set_error("%s: bad arguments", who); return JUR_EINVAL; }
  for (long e = 0; e < n; e++)
    if (iq[e] < 0 || iq[e] >= nq) { jur_set_error("%s: element %ld is of quantity %d, the box has %d", who, e, iq[e], nq); return JUR_EINVAL; }
  long count = 0;
  for (long e = 0; e < n; e++) {
    int const s = x[e] == lo[iq[e]] ? -1 : x[e] == hi[iq[e]] ? 1 : 0;
    if (side) side[e] = (signed char)s;
    count += s != 0;
  }
  return count;
}
