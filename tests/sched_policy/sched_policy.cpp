// The launch scheduler's rules (csrc/mre_policy.h) as a plain host program -- test infrastructure, not the product.
// No HIP, no Python in the process: tests/test_sched_policy.py feeds it cases on stdin and compares what it prints with
// values worked out from the rules' text; it also builds and runs under AddressSanitizer / UBSan as it stands:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       tests/sched_policy/sched_policy.cpp -o sched_policy
//
//   sched_policy decide   lines "li0 li1 li2 li3 large newton compact_only large_only"      -> "action flag_after"
//   sched_policy sort     "total lo n", total records of 4 words, total order entries        -> "kmax", the order entries
//   sched_policy tail     "total lo n", total records of 4 words                             -> "none" or the ratio
//   sched_policy free     lines "cur nyounger stage ..."                                     -> the pick
//   sched_policy window   lines "nticks queue_min_ticks tail_valid tick_tail queue_tail_min" -> 0 / 1
//   sched_policy keep     lines "nsteps ring"                                                -> launches kept unprocessed
//   sched_policy fits     lines "queue_ok queue_waves N"                                     -> 0 / 1
//   sched_policy lwaves   "n last_handovers spare_large large_waves_max", n x "li0 li1 large" -> large waves
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../mujoco_robot_environments_amd/csrc/mre_policy.h"

using namespace mre;

static bool read_records(int total, std::vector<int>& info) {
  info.resize(4 * (size_t)total);
  for (int& w : info) if (scanf("%d", &w) != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const char* mode = argv[1];
  if (!strcmp(mode, "decide")) {
    int li[4], large, newton, compact_only, large_only;
    while (scanf("%d %d %d %d %d %d %d %d", li, li + 1, li + 2, li + 3, &large, &newton, &compact_only, &large_only) == 8) {
      const policy::Action act = policy::decide(li, large != 0, newton != 0, compact_only != 0, large_only != 0);
      static const char* const names[] = {"none", "rerun", "promote", "demote", "handed_over"};
      printf("%s %d\n", names[act], (int)policy::flag_after(act, large != 0));
    }
  } else if (!strcmp(mode, "sort") || !strcmp(mode, "tail")) {
    int total, lo, n;
    std::vector<int> info;
    if (scanf("%d %d %d", &total, &lo, &n) != 3 || lo < 0 || n < 0 || lo + n > total || !read_records(total, info)) return 2;
    if (mode[0] == 's') {
      std::vector<int> order((size_t)total);
      for (int& w : order) if (scanf("%d", &w) != 1) return 2;
      printf("%d\n", policy::sort_longest_first(info.data(), lo, n, order.data()));
      for (int w : order) printf("%d ", w);
      printf("\n");
    } else {
      std::vector<int> scratch((size_t)n);
      float ratio = 0.f;
      if (policy::tick_tail_ratio(info.data(), lo, n, scratch.data(), &ratio)) printf("%.6f\n", ratio);
      else printf("none\n");
    }
  } else if (!strcmp(mode, "free")) {
    int cur, ny;
    while (scanf("%d %d", &cur, &ny) == 2) {
      int younger[policy::RING];
      if (cur < 0 || cur >= policy::NSTAGE || ny < 0 || ny >= policy::RING) return 2;
      for (int k = 0; k < ny; k++) if (scanf("%d", younger + k) != 1 || younger[k] < 0 || younger[k] >= policy::NSTAGE) return 2;
      printf("%d\n", policy::free_stage(cur, younger, ny));
    }
  } else if (!strcmp(mode, "window")) {
    int nticks, min_ticks, valid;
    float tail, tail_min;
    while (scanf("%d %d %d %f %f", &nticks, &min_ticks, &valid, &tail, &tail_min) == 5)
      printf("%d\n", (int)policy::window_wants_queue(nticks, min_ticks, valid != 0, tail, tail_min));
  } else if (!strcmp(mode, "keep")) {
    int nsteps, ring;
    while (scanf("%d %d", &nsteps, &ring) == 2) printf("%d\n", policy::ring_keep(nsteps, ring));
  } else if (!strcmp(mode, "fits")) {
    int ok, waves, N;
    while (scanf("%d %d %d", &ok, &waves, &N) == 3) printf("%d\n", (int)policy::queue_fits(ok != 0, waves, N));
  } else if (!strcmp(mode, "lwaves")) {
    int n, handovers, spare, wmax, nl = 0;
    if (scanf("%d %d %d %d", &n, &handovers, &spare, &wmax) != 4 || n < 0) return 2;
    std::vector<int> info(4 * (size_t)n, 0);
    std::vector<uint8_t> large((size_t)n);
    for (int i = 0; i < n; i++) {
      int fl;
      if (scanf("%d %d %d", &info[4 * (size_t)i], &info[4 * (size_t)i + 1], &fl) != 3) return 2;
      large[i] = fl != 0; nl += fl != 0;
    }
    printf("%d\n", policy::queue_large_waves(info.data(), large.data(), 0, n, nl, handovers, spare, wmax));
  } else {
    return 2;
  }
  return 0;
}
