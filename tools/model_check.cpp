// model_check -- the model builder (csrc/mre_model.cpp) as a plain host program: no HIP, no Python in the process,
// so it runs under the host sanitizers as it is.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/model_check.cpp mujoco_robot_environments_amd/csrc/mre_model.cpp -o model_check
//   ./model_check model.blob [ENTRY INDEX VALUE | ENTRY drop -]...
//
// model.blob is what model/compile.py's to_blob() returns.  Each triple changes one element of one entry before the
// model is built (INDEX into the flattened array; VALUE as an integer or a float, by the entry's type); `ENTRY drop -`
// renames the entry so that it is missing.  Prints "ok" or "rejected: <message>" and exits 0 either way; a sanitizer
// report ends the run with its own exit code.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../mujoco_robot_environments_amd/csrc/mre_model.h"

static unsigned char* find_entry(std::vector<unsigned char>& blob, const char* name) {
  uint32_t ne;
  memcpy(&ne, blob.data() + 8, 4);
  if (16 + 48 * (size_t)ne > blob.size()) return nullptr;
  for (uint32_t k = 0; k < ne; k++) {
    unsigned char* t = blob.data() + 16 + 48 * (size_t)k;
    if (strncmp((const char*)t, name, 32) == 0) return t;
  }
  return nullptr;
}

int main(int argc, char** argv) {
  if (argc < 2 || (argc - 2) % 3 != 0) {
    fprintf(stderr, "usage: %s model.blob [ENTRY INDEX VALUE | ENTRY drop -]...\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<unsigned char> blob;
  unsigned char buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) blob.insert(blob.end(), buf, buf + n);
  fclose(f);
  if (blob.size() < 16) { fprintf(stderr, "%s: too small for a blob\n", argv[1]); return 2; }
  for (int a = 2; a < argc; a += 3) {
    unsigned char* t = find_entry(blob, argv[a]);
    if (!t) { fprintf(stderr, "no entry %s\n", argv[a]); return 2; }
    if (strcmp(argv[a + 1], "drop") == 0) { t[0] = '~'; continue; }
    uint32_t code, count; uint64_t off;
    memcpy(&code, t + 32, 4); memcpy(&count, t + 36, 4); memcpy(&off, t + 40, 8);
    const unsigned long idx = strtoul(argv[a + 1], nullptr, 10);
    const size_t width = code ? 8 : 4;
    if (idx >= count || off + (idx + 1) * width > blob.size()) { fprintf(stderr, "%s[%lu] is out of range\n", argv[a], idx); return 2; }
    if (code) { const double v = atof(argv[a + 2]); memcpy(blob.data() + off + idx * 8, &v, 8); }
    else { const int32_t v = (int32_t)atol(argv[a + 2]); memcpy(blob.data() + off + idx * 4, &v, 4); }
  }
  mre::DevModel* m = new mre::DevModel;
  int solver = -1;
  const std::string err = mre::build_model(blob.data(), blob.size(), *m, solver);
  if (err.empty()) printf("ok (solver %d, %zu bytes of device model)\n", solver, sizeof(*m));
  else printf("rejected: %s\n", err.c_str());
  delete m;
  return 0;
}
