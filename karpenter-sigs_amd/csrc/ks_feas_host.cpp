// ks_feas_host.cpp — the static feasibility matrix on the host: the definitions of ks_feas.hip's two kernels
// (DESIGN §3 "Static feasibility matrix") in plain loops over the host images of the device tables, through
// the host side of ks_reqset.h.  No HIP call: this is the expected value the kernels are compared with.
#include "ks_feas_host.h"

#include <algorithm>

namespace ks {

std::vector<int32_t> state_pods(const Host& h) {
  std::vector<int32_t> sp((size_t)std::max(h.dims.S, 1), 0);
  for (int p = 0; p < h.dims.P; p++)
    for (int j = 0; j < h.tab.pod_nstate[(size_t)p]; j++) sp[(size_t)(h.tab.pod_state0[(size_t)p] + j)] = p;
  return sp;
}

namespace {

bool within_limits(const Host& h, int it, int pool) {
  if (pool < 0) return true;
  const int R = h.dims.R;
  const uint32_t mask = h.tab.pool_mask[(size_t)pool];
  for (int r = 0; r < R; r++)
    if (((mask >> r) & 1u) && h.tab.it_cap[(size_t)it * R + r] > h.tab.pool_rem0[(size_t)pool * R + r]) return false;
  return true;
}

bool has_offering(const Host& h, int it, const uint32_t* rs) {  // nodeclaim.go:270-278
  const auto& t = h.tab;
  for (int o = t.it_off_beg[(size_t)it]; o < t.it_off_beg[(size_t)it + 1]; o++)
    if (rs_member(h.L, rs, h.dims.zoneKey, t.off_zone[(size_t)o]) && rs_member(h.L, rs, h.dims.ctKey, t.off_ct[(size_t)o]))
      return true;
  return false;
}

}  // namespace

void static_feasibility_host(const Host& h, StaticFeas& f) {
  const KsDims& d = h.dims;
  const auto& t = h.tab;
  const int R = d.R, RSW = d.RSW;
  f.S = d.S;
  f.NTPL = d.NTPL;
  f.N = d.N;
  f.TW = d.TW;
  f.NWN = (d.N + 31) / 32;
  f.tpl_code.assign((size_t)f.S * f.NTPL, FC_NONE);
  f.tpl_count.assign((size_t)f.S * f.NTPL, 0);
  f.tpl_options.assign((size_t)f.S * f.NTPL * f.TW, 0);
  f.node_bits.assign((size_t)f.S * f.NWN, 0);
  f.node_count.assign((size_t)f.S, 0);
  const std::vector<int32_t> sp = state_pods(h);
  std::vector<uint32_t> mrg((size_t)RSW);
  std::vector<int64_t> req((size_t)R);
  for (int s = 0; s < d.S; s++) {
    const int p = sp[(size_t)s];
    const uint32_t* X = &t.st_rs[(size_t)s * RSW];
    const bool keys = (t.st_flags[(size_t)s] & SF_HAS_KEYS) != 0;
    // --- template rows: try_templates' order (ks_solve.hip)
    for (int tt = 0; tt < d.NTPL; tt++) {
      const size_t row = (size_t)s * d.NTPL + tt;
      const int tb = t.tpl_it_beg[(size_t)tt], nIT = t.tpl_it_beg[(size_t)tt + 1] - tb;
      const int pool = t.tpl_pool[(size_t)tt];
      if (pool >= 0) {
        bool any = false;
        for (int q = 0; q < nIT && !any; q++) any = within_limits(h, t.tpl_its[(size_t)(tb + q)], pool);
        if (!any) {
          f.tpl_code[row] = FC_LIMITS;
          continue;
        }
      }
      if (!((t.st_toltpl[(size_t)s] >> tt) & 1ull)) {
        f.tpl_code[row] = FC_TAINTS;
        continue;
      }
      std::copy(&t.tpl_rs[(size_t)tt * RSW], &t.tpl_rs[(size_t)tt * RSW] + RSW, mrg.begin());
      if (keys) {
        if (!rs_compatible(h.L, mrg.data(), X, d.allowWK)) {
          f.tpl_code[row] = FC_COMPAT;
          continue;
        }
        rs_add(h.L, mrg.data(), X);
      }
      for (int r = 0; r < R; r++) req[(size_t)r] = t.tpl_daemon[(size_t)tt * R + r] + t.pod_req[(size_t)p * R + r];
      uint32_t flags = 0;
      int cnt = 0;
      for (int q = 0; q < nIT; q++) {
        const int it = t.tpl_its[(size_t)(tb + q)];
        if (!within_limits(h, it, pool)) continue;
        const bool ic = rs_intersects(h.L, &t.it_rs[(size_t)it * RSW], mrg.data());
        bool fi = true;  // resources.go:162-175: a negative Allocatable never fits
        for (int r = 0; r < R; r++) {
          const int64_t a = t.it_alloc[(size_t)it * R + r];
          fi = fi && a >= 0 && req[(size_t)r] <= a;
        }
        const bool of = has_offering(h, it, mrg.data());
        if (ic) flags |= FF_REQ;
        if (fi) flags |= FF_FITS;
        if (of) flags |= FF_OFF;
        if (ic && fi && !of) flags |= FF_REQ_FITS;
        if (ic && of && !fi) flags |= FF_REQ_OFF;
        if (fi && of && !ic) flags |= FF_FITS_OFF;
        if (ic && fi && of) {
          f.tpl_options[row * f.TW + (size_t)(q >> 5)] |= 1u << (q & 31);
          cnt++;
        }
      }
      f.tpl_count[row] = cnt;
      if (cnt == 0) f.tpl_code[row] = FC_NO_IT | (flags << 8);
    }
    // --- node row: the node scan's tests on the nodes' initial state (ks_solve.hip node_okK)
    if (t.pod_flags[(size_t)p] & PF_VOLERR) continue;
    for (int n = 0; n < d.N; n++) {
      bool ok = ((t.n_taint[2 * (size_t)n] & ~t.st_tol[2 * (size_t)s]) | (t.n_taint[2 * (size_t)n + 1] & ~t.st_tol[2 * (size_t)s + 1])) == 0;
      ok = ok && (t.n_hp0[(size_t)n] & t.pod_hpc[(size_t)p]) == 0;
      for (int r = 0; r < R && ok; r++) {
        const int64_t a = t.n_avail[(size_t)n * R + r];
        ok = a >= 0 && t.n_req0[(size_t)n * R + r] + t.pod_req[(size_t)p * R + r] <= a;
      }
      if (ok && keys) ok = rs_compatible(h.L, &t.n_rs0[(size_t)n * RSW], X, 0);
      if (ok) {
        f.node_bits[(size_t)s * f.NWN + (size_t)(n >> 5)] |= 1u << (n & 31);
        f.node_count[(size_t)s]++;
      }
    }
  }
}

// Roofline convention of DESIGN §3: the table bytes a kernel addresses (a table word several rows share is
// counted for each row: the rows are independent) and the bytes of the rows it writes.
void static_feasibility_bytes(const Host& h, const StaticFeas& f, int64_t* read, int64_t* written) {
  const KsDims& d = h.dims;
  const auto& t = h.tab;
  const int64_t R = d.R, RSW = d.RSW;
  int64_t rd = 0;
  std::vector<int64_t> filt((size_t)std::max(d.NTPL, 1), 0), lim((size_t)std::max(d.NTPL, 1), 0);
  for (int tt = 0; tt < d.NTPL; tt++) {
    const int tb = t.tpl_it_beg[(size_t)tt], nIT = t.tpl_it_beg[(size_t)tt + 1] - tb;
    const bool pool = t.tpl_pool[(size_t)tt] >= 0;
    lim[(size_t)tt] = pool ? 4 + 8 * R + (int64_t)nIT * (4 + 8 * R) : 0;
    int64_t b = 16 * R;  // daemon overhead + pod requests
    for (int q = 0; q < nIT; q++) {
      const int it = t.tpl_its[(size_t)(tb + q)];
      b += 4 + 4 * RSW + 8 * R + 8 + 8 * (int64_t)(t.it_off_beg[(size_t)it + 1] - t.it_off_beg[(size_t)it]) + (pool ? 8 * R : 0);
    }
    filt[(size_t)tt] = b;
  }
  for (int s = 0; s < d.S; s++) {
    const bool keys = (t.st_flags[(size_t)s] & SF_HAS_KEYS) != 0;
    for (int tt = 0; tt < d.NTPL; tt++) {
      const uint32_t c = f.tpl_code[(size_t)s * d.NTPL + tt] & 0xffu;
      rd += 4 + 12 + 8 + lim[(size_t)tt];  // st_pod, tpl_it_beg / tpl_pool, st_toltpl
      if (c == FC_LIMITS || c == FC_TAINTS) continue;
      rd += 4 * RSW + 4 + (keys ? 4 * RSW : 0);
      if (c == FC_COMPAT) continue;
      rd += filt[(size_t)tt];
    }
    rd += 4 + 16 + 8 + 4 + 4 + 8 * R + (keys ? 4 * RSW : 0);
    rd += (int64_t)d.N * (16 + 8 + 16 * R + (keys ? 4 * RSW : 0));
  }
  *read = rd;
  *written = (int64_t)f.S * f.NTPL * (8 + 4 * (int64_t)f.TW) + (int64_t)f.S * (4 * (int64_t)f.NWN + 4);
}

}  // namespace ks
