// The pass split rule of the batch pipeline (drand_amd/csrc/hostlogic.h tail_split_main) on the
// (cnt, q) pairs of the command line, as one JSON list: tests/test_tail_split_host.py builds this under
// ASan+UBSan and compares every value with its own arithmetic. No HIP, no device.
//   tailsplit-asan CNT Q [CNT Q ...]      (decimal, up to SIZE_MAX)
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../drand_amd/csrc/hostlogic.h"

int main(int argc, char** argv) {
  if (argc < 3 || (argc - 1) % 2) {
    fprintf(stderr, "usage: %s CNT Q [CNT Q ...]\n", argv[0]);
    return 2;
  }
  std::vector<size_t> v;
  for (int k = 1; k < argc; k++) {
    char* end = nullptr;
    errno = 0;
    const unsigned long long x = strtoull(argv[k], &end, 10);
    if (end == argv[k] || *end || errno == ERANGE || x > SIZE_MAX) {
      fprintf(stderr, "bad number: %s\n", argv[k]);
      return 2;
    }
    v.push_back((size_t)x);
  }
  printf("[");
  for (size_t k = 0; k + 1 < v.size(); k += 2)
    printf("%s%zu", k ? ", " : "", blsv_detail::tail_split_main(v[k], v[k + 1]));
  printf("]\n");
  return 0;
}
