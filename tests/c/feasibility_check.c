/* feasibility_check.c — a plain C99 client of the static feasibility entries of include/karpenter_amd.h,
 * compiled with gcc (no C++, no HIP headers).
 *
 *   feasibility_check host <snapshot.json>     ks_problem_create_host + ks_problem_static_feasibility(where = 1)
 *   feasibility_check device <snapshot.json>   ks_problem_create + ks_problem_static_feasibility(where = 0)
 *
 * Walks every row through ks_feasibility_template_row / ks_feasibility_node_row and prints one JSON document:
 * {"meta": <ks_feasibility_meta>, "tpl": [[[code, count, [words]] per template] per state],
 *  "node": [[count, [words]] per state], "bytes_read", "bytes_written", "timed": kernel_ms > 0}.  Also checks that
 * out-of-range rows are KS_ERR_ARG and that ks_feasibility_free(NULL) returns.
 * tests/test_static_feasibility_host.py compares the document with the Python binding's arrays. */
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

static int fail(const char* what, int rc) {
  fprintf(stderr, "%s failed: %d %s\n", what, rc, ks_last_error());
  return 1;
}

static void put_words(const uint32_t* w, int n) {
  putchar('[');
  for (int i = 0; i < n; i++) printf(i ? ",%u" : "%u", (unsigned)w[i]);
  putchar(']');
}

int main(int argc, char** argv) {
  if (argc != 3 || (strcmp(argv[1], "host") && strcmp(argv[1], "device"))) {
    fprintf(stderr, "usage: feasibility_check host|device <snapshot.json>\n");
    return 2;
  }
  const int where = strcmp(argv[1], "host") == 0 ? 1 : 0;
  size_t len = 0;
  char* snap = slurp(argv[2], &len);
  if (!snap) {
    fprintf(stderr, "cannot read %s\n", argv[2]);
    return 2;
  }
  ks_problem* pb = NULL;
  int rc = where ? ks_problem_create_host(snap, len, &pb) : ks_problem_create(snap, len, &pb);
  if (rc != KS_OK) return fail("ks_problem_create", rc);
  ks_feasibility* f = NULL;
  if ((rc = ks_problem_static_feasibility(pb, NULL, 2, &f)) != KS_ERR_ARG) return fail("where = 2 accepted", rc);
  if ((rc = ks_problem_static_feasibility(pb, NULL, where, &f)) != KS_OK) return fail("ks_problem_static_feasibility", rc);
  ks_problem_free(pb); /* the matrix keeps what it needs */
  char* meta = NULL;
  if ((rc = ks_feasibility_meta(f, &meta)) != KS_OK) return fail("ks_feasibility_meta", rc);
  int dims[5];
  if ((rc = ks_feasibility_arrays(f, dims, NULL, NULL, NULL, NULL, NULL)) != KS_OK) return fail("ks_feasibility_arrays", rc);
  const int S = dims[0], NTPL = dims[1];
  if (ks_feasibility_template_row(f, S, 0, NULL, NULL, NULL, NULL) != KS_ERR_ARG ||
      ks_feasibility_template_row(f, 0, NTPL, NULL, NULL, NULL, NULL) != KS_ERR_ARG ||
      ks_feasibility_template_row(f, -1, 0, NULL, NULL, NULL, NULL) != KS_ERR_ARG ||
      ks_feasibility_node_row(f, S, NULL, NULL, NULL) != KS_ERR_ARG || ks_feasibility_node_row(f, -1, NULL, NULL, NULL) != KS_ERR_ARG) {
    fprintf(stderr, "an out-of-range row was accepted\n");
    return 1;
  }
  printf("{\"meta\":%s,\"tpl\":[", meta);
  ks_free(meta);
  for (int s = 0; s < S; s++) {
    printf(s ? ",[" : "[");
    for (int t = 0; t < NTPL; t++) {
      uint32_t code = 0;
      int32_t count = 0;
      const uint32_t* words = NULL;
      int nw = 0;
      if ((rc = ks_feasibility_template_row(f, s, t, &code, &count, &words, &nw)) != KS_OK) return fail("template_row", rc);
      printf(t ? ",[%u,%d," : "[%u,%d,", (unsigned)code, (int)count);
      put_words(words, nw);
      putchar(']');
    }
    putchar(']');
  }
  printf("],\"node\":[");
  for (int s = 0; s < S; s++) {
    int32_t count = 0;
    const uint32_t* words = NULL;
    int nw = 0;
    if ((rc = ks_feasibility_node_row(f, s, &count, &words, &nw)) != KS_OK) return fail("node_row", rc);
    printf(s ? ",[%d," : "[%d,", (int)count);
    put_words(words, nw);
    putchar(']');
  }
  double ms = 0;
  int64_t br = 0, bw = 0;
  if ((rc = ks_feasibility_timing(f, &ms, &br, &bw)) != KS_OK) return fail("ks_feasibility_timing", rc);
  printf("],\"bytes_read\":%lld,\"bytes_written\":%lld,\"timed\":%s}\n", (long long)br, (long long)bw, ms > 0 ? "true" : "false");
  ks_feasibility_free(f);
  ks_feasibility_free(NULL);
  free(snap);
  return 0;
}
