// policy::queue_spare_large and what it does to policy::queue_large_waves (csrc/mre_policy.h) as a plain host program --
// test infrastructure, not the product.  tests/test_queue_model_prefetch.py feeds it cases on stdin.
//   spare_policy spare    lines "last_handovers forced"                          -> spare large waves
//   spare_policy lwaves   lines "n nl last_handovers forced large_waves_max"     -> waves of the waiting large launch
//                         (n envs, the first nl flagged large, no durations recorded)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../mujoco_robot_environments_amd/csrc/mre_policy.h"

using namespace mre;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  if (!strcmp(argv[1], "spare")) {
    int handovers, forced;
    while (scanf("%d %d", &handovers, &forced) == 2) printf("%d\n", policy::queue_spare_large(handovers, forced));
  } else if (!strcmp(argv[1], "lwaves")) {
    int n, nl, handovers, forced, wmax;
    while (scanf("%d %d %d %d %d", &n, &nl, &handovers, &forced, &wmax) == 5) {
      if (n < 0 || nl < 0 || nl > n) return 2;
      std::vector<int> info(4 * (size_t)n, -1);
      std::vector<uint8_t> large((size_t)n, 0);
      for (int i = 0; i < nl; i++) large[i] = 1;
      printf("%d\n", policy::queue_large_waves(info.data(), large.data(), 0, n, nl, handovers,
                                               policy::queue_spare_large(handovers, forced), wmax));
    }
  } else {
    return 2;
  }
  return 0;
}
