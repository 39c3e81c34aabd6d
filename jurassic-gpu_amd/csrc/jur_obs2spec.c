/* jur_obs2spec.c -- `obs2spec <ctl> <obs> <spec>`: an observation file as a spectrum, one line per (ray, channel).
 *
 * What the reference's refspec example (example/refspec/run.sh) runs on every output of `formod ... TASK contrib`.
 * Layout: twelve header lines `# $1 = ..` .. `# $12 = ..`, then for every ray a blank line and one line per channel
 * with the ray's geometry (time, observer, view point, tangent point), the channel's wavenumber and its radiance
 * (brightness temperature with WRITE_BBT), formatted `%.2f %g %g %g %g %g %g %g %g %g %.4f %g`.  Host only. */
#include <stdio.h>
#include <stdlib.h>
#include "jurassic_abi.h"

#include "jur_textio.h"

int main(int argc, char *argv[]) {
  if (argc < 4) DIE("Give parameters: <ctl> <obs> <spec>");
  ctl_t *ctl = (ctl_t *)calloc(1, sizeof(ctl_t));
  obs_t *obs = (obs_t *)calloc(1, sizeof(obs_t));
  if (!ctl || !obs) DIE("Out of memory!");
  read_ctl(argc, argv, ctl);
  read_obs(argv[2], ctl, obs);
  printf("Write spectra: %s\n", argv[3]);
  FILE *out = fopen(argv[3], "w");
  if (!out) DIE("cannot write %s", argv[3]);
  fprintf(out, "# $1 = time (seconds since 2000-01-01T00:00Z)\n"
               "# $2 = observer altitude [km]\n"
               "# $3 = observer longitude [deg]\n"
               "# $4 = observer latitude [deg]\n"
               "# $5 = view point altitude [km]\n"
               "# $6 = view point longitude [deg]\n"
               "# $7 = view point latitude [deg]\n"
               "# $8 = tangent point altitude [km]\n"
               "# $9 = tangent point longitude [deg]\n"
               "# $10 = tangent point latitude [deg]\n"
               "# $11 = channel wavenumber [cm^-1]\n"
               "# $12 = channel %s\n", ctl->write_bbt ? "brightness temperature [K]" : "radiance [W/(m^2 sr cm^-1)]");
  for (int ir = 0; ir < obs->nr; ir++) {
    fprintf(out, "\n");
    for (int id = 0; id < ctl->nd; id++)
      fprintf(out, "%.2f %g %g %g %g %g %g %g %g %g %.4f %g\n", obs->time[ir], obs->obsz[ir], obs->obslon[ir],
              obs->obslat[ir], obs->vpz[ir], obs->vplon[ir], obs->vplat[ir], obs->tpz[ir], obs->tplon[ir], obs->tplat[ir],
              ctl->nu[id], obs->rad[ir][id]);
  }
  fclose(out);
  free(ctl); free(obs);
  return EXIT_SUCCESS;
}
