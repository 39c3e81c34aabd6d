/* jur_cloud.c -- cached positions of a point cloud (ctl->ip == 3), what upstream's intpol_atm_3d caches in a function
 * static on its first call (jurassic.c:766-771): x1[ip] = geo2cart(0, lon[ip], lat[ip]) of every atmosphere point.
 * Host arithmetic only: no GPU, no model. */
#include <math.h>
#include "jur_internal.h"

static void geo2cart0(double lon, double lat, double x[3]) {   /* geo2cart(0, lon, lat, x), jr_common.h:494-500 */
  double const radius = 0 + JUR_RE, deg = M_PI / 180, clat = cos(lat * deg);
  x[0] = radius * clat * cos(lon * deg);
  x[1] = radius * clat * sin(lon * deg);
  x[2] = radius * sin(lat * deg);
}

/* x1[i] for the n points (lon[i], lat[i]); returns n, or JUR_EINVAL */
long jur_cloud_rows(long n, double const *lon, double const *lat, double (*x1)[3]) {
  if (n < 1 || !lon || !lat || !x1) { jur_set_error("jur_cloud_points: no atmosphere, or no room for its positions"); return JUR_EINVAL; }
  for (long i = 0; i < n; i++) geo2cart0(lon[i], lat[i], x1[i]);
  return n;
}

long jur_cloud_points(atm_t const *atm, double (*x1)[3]) {
  if (!atm || atm->np < 1 || atm->np > JUR_NP) { jur_set_error("jur_cloud_points: need 1..%d atmospheric points", JUR_NP); return JUR_EINVAL; }
  return jur_cloud_rows(atm->np, atm->lon, atm->lat, x1);
}
