// Stand-alone driver of horn_rigid (csrc/sslam_math.hpp), the absolute-orientation solve of sslam_seg_register_pairs, on the host.
// tests/test_horn_cpu.py builds it (host side only) and compares each T with the same minimisation at 50 digits.
//
// Input (a file of whitespace-separated hex floats): rows of 16 sums in the order k_reg_sums forms them --
//   sum p (3), sum q (3), sum p q^T (9, row-major: p's coordinate is the row), the count.
// Output: per row one line of 12 hex floats, T = R row-major, then t.
#include <cstdio>
#include <cstdlib>

#include "../semantic_slam_amd/csrc/sslam_math.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char word[64];
  double s[16];
  int k = 0;
  while (fscanf(f, "%63s", word) == 1) {
    char* end = nullptr;
    s[k++] = strtod(word, &end);
    if (end == word || *end) { fprintf(stderr, "not a number: %s\n", word); return 2; }
    if (k < 16) continue;
    k = 0;
    double T[12];
    sslam::horn_rigid(s[15], s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], s[9], s[10], s[11], s[12], s[13], s[14], T);
    for (int j = 0; j < 12; ++j) printf("%a%c", T[j], j == 11 ? '\n' : ' ');
  }
  fclose(f);
  if (k) { fprintf(stderr, "short row\n"); return 2; }
  return 0;
}
