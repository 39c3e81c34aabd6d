/* jur_track.c -- profile table of a satellite track (ctl->ip == 2), what upstream's intpol_atm_2d caches in function
 * statics on its first call (jurassic.c:711-730), per time block.  Host arithmetic only: no GPU, no model. */
#include <math.h>
#include <stdlib.h>
#include "jur_internal.h"

static void geo2cart0(double lon, double lat, double x[3]) {   /* geo2cart(0, lon, lat, x), jr_common.h:494-500 */
  double const radius = 0 + JUR_RE, deg = M_PI / 180, clat = cos(lat * deg);
  x[0] = radius * clat * cos(lon * deg);
  x[1] = radius * clat * sin(lon * deg);
  x[2] = radius * sin(lat * deg);
}

/* The profiles of n atmosphere points: a profile is a maximal run of consecutive points with equal time stamp,
 * longitude and latitude; a time block is a maximal run of equal time stamps (what locate_atm hands every ray whose
 * time stamp matches one, once no run is a single point -- and a single point is a profile of one level, refused).
 * Every output may be NULL; first, len, block_of, dir hold one entry per profile (at most n / 2 + 1 are written before
 * a refusal, n / 2 without), x1 three, prof_of one per POINT.  dir: 1 / -1 the profile's altitudes strictly
 * ascend / descend, 0 neither.  Returns the number of profiles or JUR_EINVAL with upstream's words. */
long jur_track_rows(long n, double const *time, double const *z, double const *lon, double const *lat, int *first, int *len,
                    double (*x1)[3], int *block_of, int *dir, int *prof_of) {
  if (n < 1 || !time || !z || !lon || !lat) { jur_set_error("jur_track_profiles: no atmosphere"); return JUR_EINVAL; }
  long nx = 0, start = 0;
  int block = 0;
  for (long i = 0; i <= n; i++) {
    int const brk = (i == n) || (i > 0 && (time[i] != time[i - 1] || lon[i] != lon[i - 1] || lat[i] != lat[i - 1]));
    if (brk) {                                       /* the profile [start, i) is complete */
      if (i - start <= 1) { jur_set_error("Cannot identify profiles. Check ordering of data points!"); return JUR_EINVAL; }
      int const same_block = (start > 0) && (time[start] == time[start - 1]);
      if (start > 0 && !same_block) block++;
      if (same_block && fabs(lat[start - 1] - lat[start]) > 10) { jur_set_error("Distance of profiles is too large!"); return JUR_EINVAL; }
      if (first) first[nx] = (int)start;
      if (len) len[nx] = (int)(i - start);
      if (x1) geo2cart0(lon[start], lat[start], x1[nx]);
      if (block_of) block_of[nx] = block;
      if (dir) {
        int d = (z[start + 1] > z[start]) ? 1 : (z[start + 1] < z[start]) ? -1 : 0;
        for (long j = start + 2; j < i && d; j++)
          if ((d > 0) ? !(z[j] > z[j - 1]) : !(z[j] < z[j - 1])) d = 0;
        dir[nx] = d;
      }
      nx++;
      start = i;
    }
    if (i < n && prof_of) prof_of[i] = (int)nx;
  }
  return nx;
}

long jur_track_profiles(atm_t const *atm, int *first, int *len, double (*x1)[3], int *block_of) {
  if (!atm || atm->np < 1 || atm->np > JUR_NP) { jur_set_error("jur_track_profiles: need 1..%d atmospheric points", JUR_NP); return JUR_EINVAL; }
  return jur_track_rows(atm->np, atm->time, atm->z, atm->lon, atm->lat, first, len, x1, block_of, NULL, NULL);
}
