// Stand-alone driver of the request planner of the path kernels (csrc/path_rounds.hpp): reads one case, prints its rounds.
// tests/test_path_rounds_cpu.py builds it with the host compiler and compares the rounds with its own derivation.
//
// Input (whitespace-separated ints):  nx, h_xoff_col[nx];  nc, h_cparent[nc];  width fixed budget no_column fold path_cap scratch_cap;
//                                     n, then n requests of width - 4 ints.
// Output:  "refused"  or, per round,  "round m n_lds ylen_lds scr_bytes" / "up <ints>" / "src <ints>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../semantic_slam_amd/csrc/path_rounds.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  auto geti = [&]() { long long v = 0; if (fscanf(f, "%lld", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; };
  std::vector<int> xoff_col((size_t)geti());
  for (int& v : xoff_col) v = (int)geti();
  std::vector<int> cparent((size_t)geti());
  for (int& v : cparent) v = (int)geti();
  sslam::PathRules rules{};
  rules.width = (int)geti(); rules.fixed = (size_t)geti(); rules.budget = (size_t)geti();
  rules.no_column = geti() != 0; rules.fold = geti() != 0;
  rules.path_cap = (size_t)geti(); rules.scratch_cap = (size_t)geti();
  const size_t n = (size_t)geti();
  std::vector<int> reqs(n * (rules.width - 4));
  for (int& v : reqs) v = (int)geti();
  fclose(f);
  if (!sslam::path_reqs_valid(xoff_col, reqs.data(), n, rules.width, rules.no_column)) { printf("refused\n"); return 0; }
  sslam::PathRound R;
  for (size_t k0 = 0; k0 < n; k0 = R.next) {
    sslam::path_round(xoff_col, cparent, reqs.data(), n, k0, rules, R);
    printf("round %d %d %d %zu\nup", R.m, R.n_lds, R.ylen_lds, R.scr_bytes);
    for (int v : R.up) printf(" %d", v);
    printf("\nsrc");
    for (size_t v : R.src) printf(" %zu", v);
    printf("\n");
  }
  return 0;
}
