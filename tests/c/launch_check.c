/* launch_check.c — launch lists from plain C99 (gcc, include/karpenter_amd.h only).
 *
 *   launch_check layout                 prints {"sizeof_opts", "offsetof_launch_lists"} (no library call)
 *   launch_check solve <snapshot.json>  ks_problem_create + ks_solve with launch_lists set; reads every NodeClaim's
 *                                       launch list with ks_results_nodeclaim_launch and compares it, name by name,
 *                                       with "launchInstanceTypes" of the same Results' ks_results_json.  An id is
 *                                       named through the claim's own options: instance_types[k] of
 *                                       ks_results_nodeclaim is "instanceTypeOptions"[k] of the JSON.
 *                                       Prints {"claims", "entries", "over_cut", "off_rc"}; exit status 1 on any
 *                                       difference (stderr says which) or API error. */
#include <stddef.h>
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

/* The string list after the next `"key":[` at or behind *p: names[i] points at the i-th string (not terminated),
 * lens[i] is its length; instance-type names hold no quote or backslash.  Returns the count, -1 when the key or the
 * closing bracket is missing or the list is longer than cap; *p moves behind the list. */
static int string_list(const char** p, const char* key, const char** names, int* lens, int cap) {
  const char* s = strstr(*p, key);
  int n = 0;
  if (!s) return -1;
  s += strlen(key);
  while (*s && *s != ']') {
    const char* e;
    if (*s != '"') {
      s++;
      continue;
    }
    e = strchr(s + 1, '"');
    if (!e || n >= cap) return -1;
    names[n] = s + 1;
    lens[n] = (int)(e - s - 1);
    n++;
    s = e + 1;
  }
  if (*s != ']') return -1;
  *p = s + 1;
  return n;
}

int main(int argc, char** argv) {
  size_t len = 0;
  char* snap;
  char* json = NULL;
  const char* cur;
  ks_problem* pb = NULL;
  ks_results* res = NULL;
  ks_solve_opts opts;
  int nclaims, i, entries = 0, over = 0, off_rc;
  if (argc >= 2 && strcmp(argv[1], "layout") == 0) {
    printf("{\"sizeof_opts\":%d,\"offsetof_launch_lists\":%d}\n", (int)sizeof(ks_solve_opts),
           (int)offsetof(ks_solve_opts, launch_lists));
    return 0;
  }
  if (argc < 3 || strcmp(argv[1], "solve") != 0) {
    fprintf(stderr, "usage: launch_check layout | solve <snapshot.json>\n");
    return 2;
  }
  snap = slurp(argv[2], &len);
  if (!snap) {
    fprintf(stderr, "cannot read %s\n", argv[2]);
    return 2;
  }
  memset(&opts, 0, sizeof opts);
  opts.device = -1;
  opts.simulation_mode = 1;
  opts.replicas = 1;
  if (ks_problem_create(snap, len, &pb) != KS_OK) return fail("ks_problem_create");
  /* without the flag the accessor refuses */
  if (ks_solve(pb, &opts, &res) != KS_OK) return fail("ks_solve");
  off_rc = ks_results_nodeclaim_launch(res, 0, NULL, NULL, NULL, NULL);
  if (off_rc != KS_ERR_ARG || ks_results_launch_ms(res) != 0.0) {
    fprintf(stderr, "a Solve without launch_lists answered %d\n", off_rc);
    return 1;
  }
  ks_results_free(res);
  opts.launch_lists = 1;
  if (ks_solve(pb, &opts, &res) != KS_OK) return fail("ks_solve(launch_lists)");
  if (ks_results_json(res, &json) != KS_OK) return fail("ks_results_json");
  nclaims = ks_results_num_new_nodeclaims(res);
  cur = json;
  for (i = 0; i < nclaims; i++) {
    const int32_t *its = NULL, *lits = NULL, *pods = NULL;
    const double* prices = NULL;
    int tpl = 0, np = 0, nit = 0, n = 0, nopt = 0, k, q, nn, nl;
    const char** names;
    const char* lnames[100];
    int* lens;
    int llens[100];
    if (ks_results_nodeclaim(res, i, &tpl, &pods, &np, &its, &nit) != KS_OK) return fail("ks_results_nodeclaim");
    if (ks_results_nodeclaim_launch(res, i, &lits, &prices, &n, &nopt) != KS_OK) return fail("ks_results_nodeclaim_launch");
    names = (const char**)malloc(sizeof(char*) * (size_t)(nit + 1));
    lens = (int*)malloc(sizeof(int) * (size_t)(nit + 1));
    if (!names || !lens) return 1;
    nn = string_list(&cur, "\"instanceTypeOptions\":[", names, lens, nit);
    nl = string_list(&cur, "\"launchInstanceTypes\":[", lnames, llens, 100);
    if (nn != nit || nopt != nit || nl != n || n != (nit < 100 ? nit : 100)) {
      fprintf(stderr, "claim %d: %d options (JSON %d, launch accessor %d), %d launch entries (JSON %d)\n", i, nit, nn, nopt, n, nl);
      return 1;
    }
    for (k = 0; k < n; k++) {
      for (q = 0; q < nit && its[q] != lits[k]; q++) {
      }
      if (q == nit || lens[q] != llens[k] || memcmp(names[q], lnames[k], (size_t)lens[q]) != 0) {
        fprintf(stderr, "claim %d entry %d: id %d is not %.*s\n", i, k, (int)lits[k], llens[k], lnames[k]);
        return 1;
      }
      if (k && prices[k] < prices[k - 1]) {
        fprintf(stderr, "claim %d entry %d: price %g below the entry before (%g)\n", i, k, prices[k], prices[k - 1]);
        return 1;
      }
    }
    entries += n;
    over += nit > 100;
    free(names);
    free(lens);
  }
  if (ks_results_nodeclaim_launch(res, nclaims, NULL, NULL, NULL, NULL) != KS_ERR_ARG) {
    fprintf(stderr, "an index past the last NodeClaim was accepted\n");
    return 1;
  }
  printf("{\"claims\":%d,\"entries\":%d,\"over_cut\":%d,\"off_rc\":%d,\"launch_ms_positive\":%d}\n", nclaims, entries, over,
         off_rc, ks_results_launch_ms(res) > 0.0);
  ks_free(json);
  ks_results_free(res);
  ks_problem_free(pb);
  free(snap);
  return 0;
}
