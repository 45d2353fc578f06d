/* placements_check.c — the simulation commit log from plain C99 (gcc, include/karpenter_amd.h only).
 *
 *   placements_check abi                              no device: prints {"KS_CONS_PLACEMENTS", "null_handle"} (the flag's
 *                                                     value; ks_cons_sim_results' answer to a NULL handle)
 *   placements_check disrupt <snapshot.json> METHOD   ks_cons_create + ks_cons_disrupt with KS_CONS_PLACEMENTS
 *   placements_check sim <snapshot.json> SIM          ks_cons_create + ks_cons_run (world 1) + ks_cons_sim_results
 * Exit status 1 with ks_last_error() on stderr. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "karpenter_amd.h"

static char* slurp(const char* path, size_t* len) {
  FILE* f = fopen(path, "rb");
  char* buf;
  long n;
  if (!f) return NULL;
  fseek(f, 0, SEEK_END);
  n = ftell(f);
  fseek(f, 0, SEEK_SET);
  buf = (char*)malloc((size_t)n + 1);
  if (buf && fread(buf, 1, (size_t)n, f) != (size_t)n) {
    free(buf);
    buf = NULL;
  }
  fclose(f);
  if (buf) buf[n] = 0;
  *len = (size_t)n;
  return buf;
}

static int fail(const char* what) {
  fprintf(stderr, "%s: %s\n", what, ks_last_error());
  return 1;
}

int main(int argc, char** argv) {
  int (*results)(ks_cons*, int, const ks_solve_opts*, char**) = ks_cons_sim_results;
  size_t len = 0;
  char* snap;
  char* out = NULL;
  ks_cons* c = NULL;
  ks_solve_opts opts;
  memset(&opts, 0, sizeof opts);
  opts.device = -1;
  opts.simulation_mode = 1;
  opts.replicas = 1;
  if (argc >= 2 && strcmp(argv[1], "abi") == 0) {
    printf("{\"KS_CONS_PLACEMENTS\":%d,\"null_handle\":%d}\n", KS_CONS_PLACEMENTS, results(NULL, 0, &opts, &out));
    return 0;
  }
  if (argc < 4) {
    fprintf(stderr, "usage: placements_check abi | disrupt <snapshot.json> METHOD | sim <snapshot.json> SIM\n");
    return 2;
  }
  snap = slurp(argv[2], &len);
  if (!snap) {
    fprintf(stderr, "cannot read %s\n", argv[2]);
    return 2;
  }
  if (ks_cons_create(snap, len, &c) != KS_OK) return fail("ks_cons_create");
  if (strcmp(argv[1], "disrupt") == 0) {
    if (ks_cons_disrupt(c, atoi(argv[3]), &opts, KS_CONS_PLACEMENTS, &out) != KS_OK) return fail("ks_cons_disrupt");
  } else {
    double ms = 0;
    if (ks_cons_run(c, 0, 1, &opts, NULL, 0, &ms) != KS_OK) return fail("ks_cons_run");
    if (results(c, atoi(argv[3]), &opts, &out) != KS_OK) return fail("ks_cons_sim_results");
  }
  ks_cons_free(c);
  puts(out);
  ks_free(out);
  free(snap);
  return 0;
}
