/* launch_cmd_check.c — launch lists of disruption commands from plain C99 (gcc, include/karpenter_amd.h only).
 *
 *   launch_cmd_check <snapshot.json> <sim> <cons.txt> <disrupt.txt>
 *
 * ks_cons_create; ks_cons_run at world 1 with launch_lists set; ks_cons_claim_launch(sim) compared with cons.txt;
 * ks_cons_disrupt (Drift) with launch_lists set; ks_cons_disrupt_launch(0) compared with disrupt.txt.  An
 * expectation file holds "<n> <n_options>" and then n lines "<name> <price>", the price as a C99 hexadecimal
 * floating constant (exact).  Ids are named with ks_cons_instance_type_name.  Then a run and a disrupt with the flag
 * clear: both accessors must return KS_ERR_ARG.
 * Prints {"cons_entries", "disrupt_entries", "off_rc_cons", "off_rc_disrupt", "launch_ms_positive"}; exit status 1 on
 * any difference (stderr says which) or API error. */
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

/* 0 when the list (its, prices, n, nopt) is the one the file states */
static int compare(const ks_cons* c, const char* path, const int32_t* its, const double* prices, int n, int nopt) {
  FILE* f = fopen(path, "r");
  int wn = 0, wopt = 0, i, bad = 0;
  if (!f) {
    fprintf(stderr, "%s: unreadable\n", path);
    return 1;
  }
  if (fscanf(f, "%d %d", &wn, &wopt) != 2 || wn != n || wopt != nopt) {
    fprintf(stderr, "%s: %d entries of %d options, expected %d of %d\n", path, n, nopt, wn, wopt);
    bad = 1;
  }
  for (i = 0; i < n && !bad; i++) {
    char name[256], num[64];
    const char* got = ks_cons_instance_type_name(c, its[i]);
    if (fscanf(f, "%255s %63s", name, num) != 2 || !got || strcmp(got, name) != 0 || strtod(num, NULL) != prices[i]) {
      fprintf(stderr, "%s: entry %d is %s at %a\n", path, i, got ? got : "(null)", prices[i]);
      bad = 1;
    }
  }
  fclose(f);
  return bad;
}

int main(int argc, char** argv) {
  size_t len = 0;
  char* snap;
  char* js = NULL;
  ks_cons* c = NULL;
  ks_solve_opts o;
  int32_t its[100];
  double prices[100];
  const int32_t* dits = NULL;
  const double* dprices = NULL;
  int n = 0, nopt = 0, dn = 0, dnopt = 0, sim, off_cons, off_disrupt, positive;
  if (argc != 5) return 2;
  snap = slurp(argv[1], &len);
  if (!snap) return 2;
  sim = atoi(argv[2]);
  memset(&o, 0, sizeof o);
  o.device = -1;
  o.simulation_mode = 1;
  o.replicas = 1;
  o.launch_lists = 1;
  if (ks_cons_create(snap, len, &c) != KS_OK) return fail("ks_cons_create");
  if (ks_cons_run(c, 0, 1, &o, NULL, 0, NULL) != KS_OK) return fail("ks_cons_run");
  positive = ks_cons_launch_ms(c) > 0;
  if (ks_cons_claim_launch(c, sim, NULL, NULL, &n, &nopt) != KS_OK) return fail("ks_cons_claim_launch (counts)");
  if (n < 0 || n > 100) return fail("ks_cons_claim_launch: more entries than the caller's buffers hold");
  if (ks_cons_claim_launch(c, sim, its, prices, &n, &nopt) != KS_OK) return fail("ks_cons_claim_launch");
  if (compare(c, argv[3], its, prices, n, nopt)) return 1;
  if (ks_cons_claim_launch(c, sim, NULL, NULL, NULL, NULL) != KS_OK) return fail("ks_cons_claim_launch (no outputs)");
  if (ks_cons_disrupt(c, KS_DISRUPT_DRIFT, &o, 0, &js) != KS_OK) return fail("ks_cons_disrupt");
  ks_free(js);
  positive = positive && ks_cons_launch_ms(c) > 0;
  if (ks_cons_disrupt_launch(c, 0, &dits, &dprices, &dn, &dnopt) != KS_OK) return fail("ks_cons_disrupt_launch");
  if (compare(c, argv[4], dits, dprices, dn, dnopt)) return 1;
  o.launch_lists = 0;
  if (ks_cons_run(c, 0, 1, &o, NULL, 0, NULL) != KS_OK) return fail("ks_cons_run (flag clear)");
  off_cons = ks_cons_claim_launch(c, sim, its, prices, &n, &nopt);
  if (ks_cons_disrupt(c, KS_DISRUPT_DRIFT, &o, 0, &js) != KS_OK) return fail("ks_cons_disrupt (flag clear)");
  ks_free(js);
  off_disrupt = ks_cons_disrupt_launch(c, 0, &dits, &dprices, &dn, &dnopt);
  printf("{\"cons_entries\": %d, \"disrupt_entries\": %d, \"off_rc_cons\": %d, \"off_rc_disrupt\": %d, "
         "\"launch_ms_positive\": %d}\n", n, dn, off_cons, off_disrupt, positive);
  ks_cons_free(c);
  free(snap);
  return 0;
}
