/* abi_check.c — a plain C99 client of include/karpenter_amd.h, compiled with gcc (no C++, no HIP
 * headers): what a cgo shim sees of the boundary.
 *
 *   abi_check inspect <snapshot.json>   host-only encode (no device): prints the layout JSON
 *   abi_check solve <snapshot.json>     ks_problem_create + ks_solve, then every structured accessor
 *                                       (ks_results_nodeclaim / _requests / _requirements /
 *                                       existing nodes / pod errors) printed as one JSON document
 *   abi_check consolidate <snapshot.json> WORLD FLAGS MULTI SINGLE SIM_SECONDS
 *                                       one consolidation pass sharded over WORLD (<= 3) handles in this
 *                                       process, as the header describes it: ks_cons_run per rank into one
 *                                       [rank][slot] host buffer, ks_cons_needed_sims (sized by a first call),
 *                                       the requirement table read from the owners, ks_cons_decide_clock with
 *                                       the clock (MULTI, SINGLE, SIM_SECONDS) on rank 0's handle; a negative
 *                                       SIM_SECONDS means plain ks_cons_decide.  Prints the decision JSON.
 *
 * tests/test_abi_c.py builds it and checks the solve output against ks_results_json's document and the
 * consolidate output against the oracle. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "karpenter_amd.h"

static char* slurp(const char* path, size_t* len) {
  FILE* f = fopen(path, "rb");
  if (!f) return NULL;
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  char* b = (char*)malloc((size_t)n + 1);
  if (!b || fread(b, 1, (size_t)n, f) != (size_t)n) {
    fclose(f);
    free(b);
    return NULL;
  }
  b[n] = 0;
  fclose(f);
  *len = (size_t)n;
  return b;
}

static void put_str(const char* s) {  /* JSON string (the boundary's strings are UTF-8 without controls) */
  putchar('"');
  for (; *s; s++) {
    if (*s == '"' || *s == '\\') putchar('\\');
    putchar(*s);
  }
  putchar('"');
}

static int fail(const char* what, int rc) {
  fprintf(stderr, "%s failed: %d %s\n", what, rc, ks_last_error());
  return 1;
}

#define MAX_WORLD 3

/* args: WORLD FLAGS MULTI SINGLE SIM_SECONDS */
static int consolidate(const char* snap, size_t len, char** args) {
  const int world = atoi(args[0]), flags = atoi(args[1]);
  ks_cons_clock clk;
  clk.multi_timeout_s = strtod(args[2], NULL);
  clk.single_timeout_s = strtod(args[3], NULL);
  clk.sim_seconds = strtod(args[4], NULL);
  if (world < 1 || world > MAX_WORLD) {
    fprintf(stderr, "WORLD must be 1..%d\n", MAX_WORLD);
    return 2;
  }
  int rc;
  ks_cons* h[MAX_WORLD] = {NULL, NULL, NULL};
  for (int r = 0; r < world; r++)
    if ((rc = ks_cons_create(snap, len, &h[r])) != KS_OK) return fail("ks_cons_create", rc);
  /* the gathered records: [rank][slot], records_per_rank slots of record_bytes each */
  const size_t per = (size_t)ks_cons_records_per_rank(h[0], world), rb = (size_t)ks_cons_record_bytes(h[0]);
  char* recs = (char*)calloc((size_t)world * per * rb + 1, 1);
  if (!recs) return fail("calloc", 0);
  ks_solve_opts opts;
  memset(&opts, 0, sizeof opts);
  opts.device = -1;
  opts.simulation_mode = 1;
  opts.replicas = 1;
  for (int r = 0; r < world; r++) {
    double ms = 0;
    if ((rc = ks_cons_run(h[r], r, world, &opts, recs + (size_t)r * per * rb, 0, &ms)) != KS_OK)
      return fail("ks_cons_run", rc);
  }
  /* the simulations whose requirement records the output renders: the return value is the full count */
  int32_t first = -1;
  const int n = ks_cons_needed_sims(h[0], recs, world, flags, &first, 1);
  if (n < 0) return fail("ks_cons_needed_sims", n);
  int32_t* need = (int32_t*)calloc((size_t)n + 1, sizeof *need);
  if (!need) return fail("calloc", 0);
  if ((rc = ks_cons_needed_sims(h[0], recs, world, flags, need, n)) != n) return fail("ks_cons_needed_sims (2nd call)", rc);
  if (n > 0 && need[0] != first) return fail("ks_cons_needed_sims order", 0);
  /* the table, in that order; each row is read from the handle of the rank that ran the simulation */
  const size_t rsw = (size_t)ks_cons_requirement_words(h[0]);
  uint32_t* table = (uint32_t*)calloc(((size_t)n + 1) * (rsw + 1), sizeof *table);
  if (!table) return fail("calloc", 0);
  for (int i = 0; i < n; i++)
    if ((rc = ks_cons_claim_requirements(h[need[i] % world], need[i], table + (size_t)i * rsw)) != KS_OK)
      return fail("ks_cons_claim_requirements", rc);
  char* js = NULL;
  if (clk.sim_seconds < 0)
    rc = ks_cons_decide(h[0], recs, world, flags, table, &js);
  else
    rc = ks_cons_decide_clock(h[0], recs, world, flags, table, &clk, &js);
  if (rc != KS_OK) return fail("ks_cons_decide", rc);
  printf("%s\n", js);
  ks_free(js);
  free(table);
  free(need);
  free(recs);
  for (int r = 0; r < world; r++) ks_cons_free(h[r]);
  return 0;
}

int main(int argc, char** argv) {
  const int cons = argc == 8 && strcmp(argv[1], "consolidate") == 0;
  if (argc != 3 && !cons) {
    fprintf(stderr, "usage: %s inspect|solve <snapshot.json>\n       %s consolidate <snapshot.json> WORLD FLAGS MULTI SINGLE SIM_SECONDS\n",
            argv[0], argv[0]);
    return 2;
  }
  size_t len = 0;
  char* snap = slurp(argv[2], &len);
  if (!snap) {
    fprintf(stderr, "cannot read %s\n", argv[2]);
    return 2;
  }
  int rc;
  if (cons) {
    rc = consolidate(snap, len, argv + 3);
    free(snap);
    return rc;
  }
  if (strcmp(argv[1], "inspect") == 0) {
    char* dims = NULL;
    if ((rc = ks_problem_inspect(snap, len, &dims)) != KS_OK) return fail("ks_problem_inspect", rc);
    printf("%s\n", dims);
    ks_free(dims);
    free(snap);
    return 0;
  }
  ks_problem* pb = NULL;
  if ((rc = ks_problem_create(snap, len, &pb)) != KS_OK) return fail("ks_problem_create", rc);
  ks_solve_opts opts;
  memset(&opts, 0, sizeof opts);
  opts.device = -1;
  opts.simulation_mode = 1;
  ks_results* r = NULL;
  if ((rc = ks_solve(pb, &opts, &r)) != KS_OK) return fail("ks_solve", rc);
  printf("{\"newNodeClaims\":[");
  int nc = ks_results_num_new_nodeclaims(r);
  for (int i = 0; i < nc; i++) {
    int tpl = -1, np = 0, nit = 0, nq = 0, nr = 0;
    const int32_t *pods = NULL, *its = NULL;
    const char *const *names = NULL, *const *qty = NULL;
    const ks_requirement* reqs = NULL;
    if ((rc = ks_results_nodeclaim(r, i, &tpl, &pods, &np, &its, &nit)) != KS_OK) return fail("ks_results_nodeclaim", rc);
    if ((rc = ks_results_nodeclaim_requests(r, i, &nq, &names, &qty)) != KS_OK) return fail("ks_results_nodeclaim_requests", rc);
    if ((rc = ks_results_nodeclaim_requirements(r, i, &nr, &reqs)) != KS_OK)
      return fail("ks_results_nodeclaim_requirements", rc);
    printf("%s{\"template\":%d,\"pods\":[", i ? "," : "", tpl);
    for (int k = 0; k < np; k++) printf("%s%d", k ? "," : "", pods[k]);
    printf("],\"instanceTypes\":[");
    for (int k = 0; k < nit; k++) printf("%s%d", k ? "," : "", its[k]);
    printf("],\"requests\":{");
    for (int k = 0; k < nq; k++) {
      if (k) putchar(',');
      put_str(names[k]);
      putchar(':');
      put_str(qty[k]);
    }
    printf("},\"requirements\":[");
    for (int k = 0; k < nr; k++) {
      printf("%s{\"key\":", k ? "," : "");
      put_str(reqs[k].key);
      printf(",\"op\":");
      put_str(reqs[k].op);
      printf(",\"values\":[");
      for (int v = 0; v < reqs[k].n_values; v++) {
        if (v) putchar(',');
        put_str(reqs[k].values[v]);
      }
      printf("]");
      if (reqs[k].has_gt) printf(",\"gt\":%lld", (long long)reqs[k].gt);
      if (reqs[k].has_lt) printf(",\"lt\":%lld", (long long)reqs[k].lt);
      printf("}");
    }
    printf("]}");
  }
  printf("],\"existingNodes\":[");
  int nn = ks_results_num_existing_nodes(r);
  for (int i = 0; i < nn; i++) {
    int idx = -1, np = 0;
    const int32_t* pods = NULL;
    if ((rc = ks_results_existing_node(r, i, &idx, &pods, &np)) != KS_OK) return fail("ks_results_existing_node", rc);
    printf("%s{\"stateNode\":%d,\"pods\":[", i ? "," : "", idx);
    for (int k = 0; k < np; k++) printf("%s%d", k ? "," : "", pods[k]);
    printf("]}");
  }
  printf("],\"podErrors\":{");
  int ne = ks_results_num_pod_errors(r);
  for (int i = 0; i < ne; i++) {
    int pod = -1;
    const char* msg = NULL;
    if ((rc = ks_results_pod_error(r, i, &pod, &msg)) != KS_OK) return fail("ks_results_pod_error", rc);
    printf("%s\"%d\":", i ? "," : "", pod);
    put_str(msg);
  }
  printf("},\"kernelMs\":%.6f}\n", ks_results_kernel_ms(r));
  /* out-of-range accessors are argument errors, not crashes */
  if (ks_results_nodeclaim(r, nc, NULL, NULL, NULL, NULL, NULL) != KS_ERR_ARG) return fail("range check", 0);
  ks_results_free(r);
  ks_problem_free(pb);
  free(snap);
  return 0;
}
