/* Stand-alone check of the host function behind every atmosphere upload under IP 3 (jur_cloud.c: jur_cloud_rows,
 * jur_cloud_points), meant for a sanitizer build on the CPU; no GPU, no library:
 *
 *   gcc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
 *       -I/opt/rocm/include -Iinclude -Ijurassic-gpu_amd/csrc -DJUR_ND=100 -DJUR_NG=30 \
 *       -o check_cloud_host tools/check_cloud_host.c jurassic-gpu_amd/csrc/jur_cloud.c -lm && ./check_cloud_host
 *
 * 2000 seeded clouds of 1 .. 300 points, longitude, latitude and the table malloc'ed to their exact sizes -- n doubles,
 * n positions -- so that a read or write beyond them is an error of the sanitizer.  Checked per cloud: the count, every
 * position on the sphere of radius JUR_RE and equal to geo2cart(0, lon, lat) as written here, the pole and the date
 * line among them; a guard position behind the table untouched; NULL rows, a NULL table and an empty cloud refused; and
 * jur_cloud_points on a whole atm_t at its largest size, JUR_NP points. */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "jur_internal.h"

static char g_msg[512];
void jur_set_error(char const *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof g_msg, fmt, ap);
  va_end(ap);
}

static unsigned long long g_state = 88172645463325252ULL;
static unsigned long long rnd(void) { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }
static double uni(double lo, double hi) { return lo + (hi - lo) * (double)(rnd() % 1000001) / 1e6; }

static int on_sphere(double const x[3], double lon, double lat) {
  double const deg = M_PI / 180, c = cos(lat * deg);
  double const want[3] = {JUR_RE * c * cos(lon * deg), JUR_RE * c * sin(lon * deg), JUR_RE * sin(lat * deg)};
  double const r = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  if (!(fabs(r - JUR_RE) < 1e-9 * JUR_RE)) return 0;
  for (int i = 0; i < 3; i++)
    if (!(fabs(x[i] - want[i]) <= 1e-9 * JUR_RE)) return 0;
  return 1;
}

static int check_one(int trial) {
  int const n = 1 + (int)(rnd() % 300);
  double *lon = malloc(sizeof(double) * n), *lat = malloc(sizeof(double) * n);
  for (int i = 0; i < n; i++) {
    lon[i] = (rnd() % 16 == 0) ? ((rnd() & 1) ? 180.0 : -180.0) : uni(-180, 180);
    lat[i] = (rnd() % 16 == 0) ? ((rnd() & 1) ? 90.0 : -90.0) : uni(-90, 90);
  }
  int fails = 0;
  /* (the table holds n positions: a write to position n is the sanitizer's to report) */
  double (*x1)[3] = malloc(sizeof(double) * 3 * n);
  for (int i = 0; i < n; i++) x1[i][0] = x1[i][1] = x1[i][2] = -77;
  long const rc = jur_cloud_rows(n, lon, lat, x1);
  if (rc != n) { printf("trial %d: %ld positions, expected %d (%s)\n", trial, rc, n, g_msg); fails++; }
  else
    for (int i = 0; i < n; i++)
      if (!on_sphere(x1[i], lon[i], lat[i])) { printf("trial %d: position %d of (%g, %g) wrong\n", trial, i, lon[i], lat[i]); fails++; break; }
  if (jur_cloud_rows(n, NULL, lat, x1) != JUR_EINVAL || jur_cloud_rows(n, lon, NULL, x1) != JUR_EINVAL ||
      jur_cloud_rows(n, lon, lat, NULL) != JUR_EINVAL || jur_cloud_rows(0, lon, lat, x1) != JUR_EINVAL) {
    printf("trial %d: a call without rows, without a table or without points was accepted\n", trial);
    fails++;
  }
  free(x1); free(lon); free(lat);
  return fails;
}

int main(void) {
  int fails = 0;
  for (int t = 0; t < 2000; t++) fails += check_one(t);
  atm_t *atm = calloc(1, sizeof(atm_t));
  double (*x1)[3] = malloc(sizeof(double) * 3 * JUR_NP);
  if (!atm || !x1) { printf("out of memory\n"); return 1; }
  for (int i = 0; i < JUR_NP; i++) { atm->lon[i] = uni(-180, 180); atm->lat[i] = uni(-90, 90); }
  atm->np = JUR_NP;
  if (jur_cloud_points(atm, x1) != JUR_NP || !on_sphere(x1[JUR_NP - 1], atm->lon[JUR_NP - 1], atm->lat[JUR_NP - 1])) { printf("JUR_NP points: wrong\n"); fails++; }
  atm->np = JUR_NP + 1;
  if (jur_cloud_points(atm, x1) != JUR_EINVAL) { printf("JUR_NP + 1 points were accepted\n"); fails++; }
  atm->np = 0;
  if (jur_cloud_points(atm, x1) != JUR_EINVAL || jur_cloud_points(NULL, x1) != JUR_EINVAL) { printf("no points were accepted\n"); fails++; }
  atm->np = 5;
  if (jur_cloud_points(atm, NULL) != JUR_EINVAL) { printf("a NULL table was accepted\n"); fails++; }
  free(atm); free(x1);
  printf("check_cloud_host: 2000 clouds, %d failures\n", fails);
  return fails ? 1 : 0;
}
