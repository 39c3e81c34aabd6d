/* jur_cli.c -- `formod <ctl> <obs> <atm> <rad> [KEY VALUE]...` on top of libjurassic_hip.so.
 *
 * The reference's forward-model executable (formod.c:33-69) so that its example scripts can call this
 * library's formod() unchanged; text I/O in jur_textio.c.  Everything numerical happens behind formod().
 * TASK contrib (the refspec example) writes <rad> and, through formod_contrib(), <rad>.<EMITTER> for every
 * emitter and <rad>.EXTINCT; any other TASK is the plain forward model.
 */
#include <stdio.h>
#include <stdlib.h>
#include <strings.h>
#include "jurassic_hip.h"

#include "jur_textio.h"

int main(int argc, char *argv[]) {
  if (argc < 5) DIE("Give parameters: <ctl> <obs> <atm> <rad>");
  ctl_t *ctl = (ctl_t *)calloc(1, sizeof(ctl_t));
  atm_t *atm = (atm_t *)calloc(1, sizeof(atm_t));
  obs_t *obs = (obs_t *)calloc(1, sizeof(obs_t));
  if (!ctl || !atm || !obs) DIE("Out of memory!");
  static char task[JUR_LEN];
  scan_ctl(argc, argv, "TASK", -1, "-", task);
  read_ctl(argc, argv, ctl);
  read_obs(argv[2], ctl, obs);
  read_atm(argv[3], ctl, atm);
  if (0 == strcasecmp(task, "contrib")) {
    obs_t *contrib = (obs_t *)calloc((size_t)ctl->ng + 1, sizeof(obs_t));
    if (!contrib) DIE("Out of memory!");
    formod_contrib(ctl, atm, obs, contrib);
    write_obs(argv[4], ctl, obs);
    static char name[2 * JUR_LEN];
    for (int v = 0; v <= ctl->ng; v++) {
      snprintf(name, sizeof name, "%s.%s", argv[4], v < ctl->ng ? ctl->emitter[v] : "EXTINCT");
      write_obs(name, ctl, &contrib[v]);
    }
    free(contrib);
  } else {
    formod(ctl, atm, obs);
    write_obs(argv[4], ctl, obs);
  }
  free(ctl); free(atm); free(obs);
  return EXIT_SUCCESS;
}
