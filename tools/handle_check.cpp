// handle_check -- the handle's life cycle (csrc/mre_api.cpp: mre_create, mre_destroy) as a plain host program on a machine
// WITHOUT a GPU: no Python in the process, so the host units run under the host sanitizers as they are.
//
//   C=mujoco_robot_environments_amd/csrc; S="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
//   for u in api sched model; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC $S -c $C/mre_$u.cpp -o /tmp/$u.san.o; done
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c tools/handle_check.cpp -o /tmp/handle_check.o
//   hipcc --offload-arch=gfx950 $S /tmp/handle_check.o /tmp/{api,sched,model}.san.o \
//       $(ls $C/_build/*.o | grep -v -e /api.o -e /sched.o -e /model.o) -o handle_check
//   ./handle_check model.blob
//
// (the other units of the library, the kernels and their launchers, come from the product build's objects as they are).
// model.blob is what model/compile.py's to_blob() returns.  Three calls: mre_create on a truncated blob (MRE_ERR_MODEL, the
// handle is deleted before any HIP call), mre_create on the good blob with no device visible (MRE_ERR_NOGPU, the handle is
// deleted with nothing to release), mre_destroy(NULL).  Prints what each answered and exits 0 when all three answered that;
// a sanitizer report ends the run with its own exit code.
#include <cstdio>
#include <vector>

#include "../include/mre.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s model.blob\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<unsigned char> blob;
  unsigned char buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) blob.insert(blob.end(), buf, buf + n);
  fclose(f);
  mre_env* e = (mre_env*)buf;   // (every call must set it to NULL)
  const int bad = mre_create(blob.data(), blob.size() / 2, 3, 0, &e);
  printf("mre_create, half the blob: %d (%s), handle %p\n", bad, mre_last_error(), (void*)e);
  int ok = bad == MRE_ERR_MODEL && e == nullptr;
  e = (mre_env*)buf;
  const int nogpu = mre_create(blob.data(), blob.size(), 3, 0, &e);
  printf("mre_create, no device: %d (%s), handle %p\n", nogpu, mre_last_error(), (void*)e);
  ok = ok && nogpu == MRE_ERR_NOGPU && e == nullptr;
  const int none = mre_destroy(nullptr);
  printf("mre_destroy(NULL): %d\n", none);
  return ok && none == MRE_OK ? 0 : 1;
}
