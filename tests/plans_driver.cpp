// Test driver of diaglib_amd/csrc/hip_plans.h, built with g++ and no ROCm include (tests/test_plans.py): reads one request per
// line from standard input and prints, per request, the plan's fields as key=value
// tokens and, behind " | ", the name the engine would book for the launch.
//
//   env NCU LDS_LIMIT T0 .. T7                      the device and the knobs of the requests that follow
//   policy DROP_FINAL PUBLISH_PENDING BASIS_EXACT CHAIN_OFF DROP_TOL
//   gram N L K SAME ALIGNED LOWER
//   wp N M K PROJECT                   wp_lds N M K PROJECT: WpPlan::lds_bytes alone
//   gemm N L K MODE FUSE PACKED_ON_DEVICE VEC2
//   ritz N L M K2 VEC2 NSLOTS          ritz2 N L M VEC2 NSLOTS
//   chain M K VEC2 BX_IS_X COMBO_OK HOST_BETWEEN X3_COOLDOWN DMAT_COLS DMAT_NONTRIVIAL FUSED_LDS_KK
//   default K M FOLD VSX WIDE_GRAMX WIDE_XW DROPF X3          (a ChainShape)
//   lean M K P2P_ON NRANKS COMM
//   close LEAN X3 OP ...
//   fused L K                          fused_lds
//   instances                          the instance lists on one line, and gram_direct_instance over tlw 1..12 x kt 1..4
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../diaglib_amd/csrc/hip_plans.h"

using namespace dla_plans;

static void print_ops(const std::vector<int>& plan)
{
  std::printf("ops=");
  for (size_t i = 0; i < plan.size(); ++i) std::printf(i ? ",%d" : "%d", plan[i]);
  std::printf("\n");
}

int main()
{
  std::istream& in = std::cin;
  Knobs knobs;
  int ncu = 256;
  size_t lds_limit = (size_t)160 * 1024;
  dla::ChainPolicy policy;
  std::string line, what;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    if (!(ss >> what)) continue;
    const PlanEnv env{ncu, lds_limit, knobs};
    if (what == "env") {
      ss >> ncu >> lds_limit;
      for (int i = 0; i < 8; ++i) { int v = 0; ss >> v; knobs.set(i, v); }
    } else if (what == "policy") {
      ss >> policy.drop_final >> policy.publish_pending >> policy.basis_exact >> policy.chain_off >> policy.drop_tol;
    } else if (what == "gram") {
      int n, l, k; bool same, aligned, lower;
      ss >> n >> l >> k >> same >> aligned >> lower;
      const GramPlan p = gram_plan(env, n, l, k, same, aligned, lower);
      std::printf("tlw=%d kt=%d px=%d passes=%d rows=%d lds=%d self=%d qt=%d low_single=%d lower=%d blocks_per_pass=%d vec2=%d lds_bytes=%zu can32=%d | %s\n",
                  p.tlw, p.kt, p.px, p.passes, p.rows, p.lds, p.self, p.qt, p.low_single, p.lower, p.blocks_per_pass, p.vec2, p.lds_bytes(),
                  gram_can32(p.tlw, p.kt) ? 1 : 0, p.name().c_str());
    } else if (what == "wp") {
      int n, m, k; bool project;
      ss >> n >> m >> k >> project;
      const WpPlan p = wp_plan(env, n, m, k, project);
      std::printf("tlw=%d kt=%d R=%d passes=%d blocks=%d extra=%d slots=%d self=%d max_tlw=%d | %s\n", p.tlw, p.kt, p.R, p.passes, p.blocks, p.extra,
                  p.slots, p.self, wp_max_tlw(p.kt), p.name().c_str());
    } else if (what == "wp_lds") {
      int n, m, k; bool project;
      ss >> n >> m >> k >> project;
      std::printf("lds_bytes=%zu\n", wp_plan(env, n, m, k, project).lds_bytes());
    } else if (what == "gemm") {
      int n, l, k, mode; bool fuse, packed, vec2;
      ss >> n >> l >> k >> mode >> fuse >> packed >> vec2;
      const GemmPlan p = gemm_plan(env, n, l, k, mode, fuse, packed, vec2);
      std::printf("kt=%d l4=%d inl=%d qt=%d lds=%zu per_cu=%d rtp=%d pipe=%d blocks=%d | %s\n", p.kt, p.l4, p.inl, p.qt, p.lds, p.per_cu, p.rtp, p.pipe,
                  p.blocks, p.name().c_str());
    } else if (what == "ritz") {
      int n, l, m, k2, nslots; bool vec2;
      ss >> n >> l >> m >> k2 >> vec2 >> nslots;
      const RitzPlan p = ritz_plan(env, n, l, m, k2, vec2, nslots);
      std::printf("kt=%d l4=%d qt=%d xp=%d pipe=%d lds_c=%zu fits=%d lds=%zu per_cu=%d blocks=%d dyn_limit=%zu | %s\n", p.kt, p.l4, p.qt, p.xp, p.pipe,
                  p.lds_c, p.fits, p.lds, p.per_cu, p.blocks, ritz_dyn_limit(env, p.kt), p.name().c_str());
    } else if (what == "ritz2") {
      int n, l, m, nslots; bool vec2;
      ss >> n >> l >> m >> vec2 >> nslots;
      const Ritz2Plan p = ritz2_plan(env, n, l, m, vec2, nslots);
      std::printf("kt=%d l4=%d lds_c=%zu fits=%d lds=%zu per_cu=%d blocks=%d | %s\n", p.kt, p.l4, p.lds_c, p.fits, p.lds, p.per_cu, p.blocks,
                  p.name().c_str());
    } else if (what == "chain") {
      ChainIn c{};
      ss >> c.m >> c.k >> c.vec2 >> c.bx_is_x >> c.combo_ok >> c.host_between >> c.x3_cooldown >> c.dmat_cols >> c.dmat_nontrivial >> c.fused_lds_kk;
      const ChainChoice ch = chain_choice(env, policy, c);
      std::printf("take=%s fold=%d x3=%d wide_gramx=%d wide_xw=%d\n", ch.take == ChainChoice::chain ? "chain" : ch.take == ChainChoice::host_loop ? "host_loop" : "nothing",
                  ch.fold, ch.x3, ch.wide_gramx, ch.wide_xw);
    } else if (what == "default") {
      ChainShape s;
      ss >> s.k >> s.m >> s.fold >> s.vsx >> s.wide_gramx >> s.wide_xw >> s.dropf >> s.x3;
      print_ops(default_plan(s));
    } else if (what == "lean") {
      int m, k, nranks; bool p2p_on, comm;
      ss >> m >> k >> p2p_on >> nranks >> comm;
      std::printf("lean=%d\n", chain_lean(env, policy, m, k, Transport{p2p_on, nranks, comm}) ? 1 : 0);
    } else if (what == "close") {
      bool lean, x3; int op;
      std::vector<int> plan;
      ss >> lean >> x3;
      while (ss >> op) plan.push_back(op);
      print_ops(close_plan(plan, lean, x3));
    } else if (what == "fused") {
      int l, k;
      ss >> l >> k;
      std::printf("fused_lds=%zu\n", fused_lds(l, k));
    } else if (what == "instances") {
      std::printf("gram_tiles=");
      for (const GramTile& t : GRAM_TILES) std::printf("%d,%d;", t.tlw, t.kt);
      std::printf(" gram_direct=");
      for (int t = 1; t <= 12; ++t)
        for (int k = 1; k <= 4; ++k) if (gram_direct_instance(t, k)) std::printf("%d,%d;", t, k);
      std::printf(" gram_low_tiles=");
      for (int t : GRAM_LOW_TILES) std::printf("%d;", t);
      std::printf(" wp_tiles=");
      for (const WpTile& t : WP_TILES) std::printf("%d,%d,%d;", t.tlw, t.kt, t.R);
      std::printf(" gram_lds_forms=");
      for (const GramLdsForm& f : GRAM_LDS_FORMS) std::printf("%d,%d;", f.self, f.qt);
      std::printf(" gemm=");
      for (const GemmInstance& g : GEMM_INSTANCES.row) std::printf("%d,%d,%d,%d,%d,%d,%d,%d;", g.kt, g.vec, g.mode, g.inl, g.fuse, g.pipe, g.qt, g.rtp);
      std::printf(" ritz_instances=");
      for (const RitzInstance& r : RITZ_INSTANCES) std::printf("%d,%d,%d,%d,%d;", r.kt, r.vec, r.pipe, r.qt, r.xp ? 1 : 0);
      std::printf(" ritz2_instances=");
      for (const Ritz2Instance& r : RITZ2_INSTANCES) std::printf("%d,%d;", r.kt, r.vec);
      std::printf("\n");
    } else {
      std::fprintf(stderr, "unknown request: %s\n", line.c_str());
      return 2;
    }
    if (what != "close" && ss.fail()) { std::fprintf(stderr, "bad request: %s\n", line.c_str()); return 2; }
  }
  std::printf("ops: NONE=%d GRAM_UU=%d TRMMG=%d XU=%d COMBO=%d FINAL=%d GRAMX=%d GRAMW=%d XW=%d COMBOX=%d CLOSE=%d TRMMC=%d\n", OP_NONE, OP_GRAM_UU,
              OP_TRMMG, OP_XU, OP_COMBO, OP_FINAL, OP_GRAMX, OP_GRAMW, OP_XW, OP_COMBOX, OP_CLOSE, OP_TRMMC);
  return 0;
}
