// Prints what a launch of the Kronecker Gram kernel decides on the host (csrc/kp_gram3_launch.h): form, geometry and the "what
// ran" timer values, for facts and switches given as arguments, host only:
//   g++ -std=c++17 -O1 -I koopman-realizations_amd/csrc tools/gram3_launch_check.cpp -o gram3_launch_check
//   gram3_launch_check name=value ...
// Facts, by the field names of Gram3Facts (unnamed ones keep 0 / false; wg_per_cu keeps 2): N m nfull nzeta k_pcs pow_depth fast
// fast_ext ext_Dp ext_df ext_ng lift_table nq nsuper njobs two_group_jobs other_nq other_nsuper other_njobs Ns n num_cu wg_per_cu
// hbm_bytes; buffer_ok (default 1): whether the prelift buffer can be had; max_kps (default 512): KP_GRAM_GROUP_MAX_KPS.
// Switches, by the names of their environment variables, with the text the library would read: KP_NO_GRAM3_EXT
// KP_GRAM3_NO_PRELIFT KP_GRAM3_PRELIFT_MIN_NS KP_GRAM3_POW3 KP_GRAM3_LIFT_ORDER KP_GRAM3_EARLY_BARRIER.
// `timing=1` prints instead gram3_tile_timing(nq, lo, eb) for nq = 1 .. 6, lo and eb 0 / 1.
// One line of JSON.  tests/test_gram3_launch_plan.py runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>

#include "kp_gram3_launch.h"

int main(int argc, char** argv) {
  std::map<std::string, std::string> arg;
  for (int i = 1; i < argc; ++i) {
    const char* eq = strchr(argv[i], '=');
    if (!eq || eq == argv[i]) {
      fprintf(stderr, "%s: %s: not name=value\n", argv[0], argv[i]);
      return 2;
    }
    arg[std::string(argv[i], eq - argv[i])] = eq + 1;
  }
  std::set<std::string> used;
  auto take = [&](const char* name) -> const char* {
    auto it = arg.find(name);
    if (it == arg.end()) return nullptr;
    used.insert(it->first);
    return it->second.c_str();
  };
  auto num = [&](const char* name, long long dflt) { const char* t = take(name); return t ? atoll(t) : dflt; };

  if (num("timing", 0)) {
    printf("{\"timing\": [");
    for (int nq = 1; nq <= 6; ++nq)
      for (int lo = 0; lo < 2; ++lo)
        for (int eb = 0; eb < 2; ++eb) {
          const Gram3TileTiming t = gram3_tile_timing(nq, lo != 0, eb != 0);
          printf("%s{\"nq\": %d, \"lo\": %d, \"eb\": %d, \"pf\": %d, \"sp\": %d, \"lag\": %d, \"bs\": %d}", nq + lo + eb > 1 ? ", " : "", nq, lo, eb, t.pf, t.sp, t.lag, t.bs);
        }
    printf("]}\n");
    return 0;
  }

  Gram3Facts f;
  f.N = (int)num("N", 0); f.m = (int)num("m", 0); f.nfull = (int)num("nfull", 0); f.nzeta = (int)num("nzeta", 0);
  f.k_pcs = (int)num("k_pcs", 0); f.pow_depth = (int)num("pow_depth", 0);
  f.fast = num("fast", 0) != 0; f.fast_ext = num("fast_ext", 0) != 0;
  f.ext_Dp = (int)num("ext_Dp", 0); f.ext_df = (int)num("ext_df", 0); f.ext_ng = (int)num("ext_ng", 0);
  f.lift_table = num("lift_table", 0) != 0;
  f.nq = (int)num("nq", 0); f.nsuper = (int)num("nsuper", 0); f.njobs = (int)num("njobs", 0); f.two_group_jobs = (int)num("two_group_jobs", 0);
  f.other_nq = (int)num("other_nq", 0); f.other_nsuper = (int)num("other_nsuper", 0); f.other_njobs = (int)num("other_njobs", 0);
  f.Ns = num("Ns", 0); f.n = (int)num("n", 1);
  f.num_cu = (int)num("num_cu", 0); f.wg_per_cu = (int)num("wg_per_cu", 2); f.hbm_bytes = num("hbm_bytes", 0);
  const bool buffer_ok = num("buffer_ok", 1) != 0;
  const long long max_kps = num("max_kps", 512);
  const Gram3Switches sw = gram3_switches_read(take);
  for (const auto& kv : arg)
    if (!used.count(kv.first)) {
      fprintf(stderr, "%s: %s: not a fact or a switch\n", argv[0], kv.first.c_str());
      return 2;
    }
  // what the launcher has checked, or its plans guarantee, before it asks
  if (f.N < 1 || f.m < 1 || f.m > 3 || f.nq < 1 || f.nq > 6 || f.nsuper < 1 || f.njobs != 4 * f.nsuper || f.Ns < 0 || f.n < 1 || f.n > 8 || f.wg_per_cu < 1 ||
      f.other_nsuper < 0) {
    fprintf(stderr, "%s: not a launch (N >= 1, 1 <= m <= 3, 1 <= nq <= 6, nsuper >= 1, njobs = 4 nsuper, Ns >= 0, 1 <= n <= 8, wg_per_cu >= 1)\n", argv[0]);
    return 2;
  }

  const Gram3Form ask = gram3_form(f, sw, true);
  const Gram3Form F = ask.want_buffer && !buffer_ok ? gram3_form(f, sw, false) : ask;
  static const char* const kinds[] = {"mono", "pcs", "ext", "pre"};
  printf("{\"form\": {\"kind\": \"%s\", \"ext\": %s, \"nq\": %d, \"bm\": %d, \"p3\": %s, \"lo\": %s, \"eb\": %s, \"want_buffer\": %s, \"pre_bytes\": %zu, \"pre_rl\": %d, \"refusal\": ",
         kinds[F.kind], F.ext ? "true" : "false", F.nq, F.bm, F.p3 ? "true" : "false", F.lo ? "true" : "false", F.eb ? "true" : "false",
         F.want_buffer ? "true" : "false", F.pre_bytes, F.pre_rl);
  if (F.refusal) printf("\"%s\"}", F.refusal);
  else printf("null}");
  const Gram3Geometry g = gram3_geometry(f);
  Gram3Facts lone = f;
  lone.n = 1;
  printf(", \"geometry\": {\"ktiles\": %lld, \"nsplit\": %d, \"kps\": %d, \"grid\": %d, \"part_bytes\": %zu, \"ws4_bytes\": %zu, \"lds\": %zu, \"reduce_block\": %d, "
         "\"slots\": %lld, \"lone_splits_shorter\": %s}",
         (long long)g.ktiles, g.nsplit, g.kps, g.grid, g.part_bytes, g.ws4_bytes, gram3_lds_bytes(f, F), g.reduce_block, (long long)gram3_slots(f),
         gram3_lone_splits_shorter(lone, max_kps) ? "true" : "false");
  const Gram3Ran r = gram3_ran(f, F);
  printf(", \"timers\": {\"10\": %.1f, \"15\": %.1f, \"16\": %.1f, \"20\": %.1f, \"26\": %.1f}}\n", r.mfma_flop_per_pair, r.two_group_jobs, r.table_entries, r.lift_order,
         r.early_barrier);
  return 0;
}
