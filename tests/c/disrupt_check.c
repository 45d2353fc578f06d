/* disrupt_check.c — Drift / Expiration from plain C99 (gcc, include/karpenter_amd.h only).
 *
 *   disrupt_check inspect <snapshot.json> METHOD         ks_cons_inspect_disrupt (host-only): prints its JSON
 *   disrupt_check disrupt <snapshot.json> METHOD FLAGS   ks_cons_create + ks_cons_disrupt: prints the command JSON
 * METHOD: KS_DISRUPT_EXPIRATION (1) or KS_DISRUPT_DRIFT (2).  Exit status 1 with ks_last_error() on stderr. */
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
  size_t len = 0;
  char* snap;
  char* out = NULL;
  int method;
  if (argc < 4) {
    fprintf(stderr, "usage: disrupt_check inspect|disrupt <snapshot.json> METHOD [FLAGS]\n");
    return 2;
  }
  snap = slurp(argv[2], &len);
  if (!snap) {
    fprintf(stderr, "cannot read %s\n", argv[2]);
    return 2;
  }
  method = atoi(argv[3]);
  if (method != KS_DISRUPT_EXPIRATION && method != KS_DISRUPT_DRIFT) return 2;
  if (strcmp(argv[1], "inspect") == 0) {
    if (ks_cons_inspect_disrupt(snap, len, NULL, 0, method, &out) != KS_OK) return fail("ks_cons_inspect_disrupt");
  } else {
    ks_cons* c = NULL;
    ks_solve_opts opts;
    memset(&opts, 0, sizeof opts);
    opts.device = -1;
    opts.simulation_mode = 1;
    opts.replicas = 1;
    if (ks_cons_create(snap, len, &c) != KS_OK) return fail("ks_cons_create");
    if (ks_cons_disrupt(c, method, &opts, argc > 4 ? atoi(argv[4]) : 0, &out) != KS_OK) return fail("ks_cons_disrupt");
    ks_cons_free(c);
  }
  puts(out);
  ks_free(out);
  free(snap);
  return 0;
}
