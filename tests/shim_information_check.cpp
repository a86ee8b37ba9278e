// The C++ shim's InformationMatrixCalculator (include/ps_graph_slam_amd/information_matrix_calculator.hpp): the fitness score and the
// information matrix of two small clouds, through a cloud type with .points[i].x/.y/.z and an Eigen-like pose as well as through plain
// arrays.  Without a GPU the program checks the host side only; with one it prints the score and the 36 numbers that
// tests/test_fitness_gpu.py compares, bitwise, with the Python mirror.  The clouds are rebuilt there by _shim_clouds(): keep the two in step.
#include <cmath>
#include <cstdio>
#include <vector>
#include "../include/ps_graph_slam_amd/information_matrix_calculator.hpp"

struct Point { float x, y, z; };
struct Cloud { std::vector<Point> points; };
struct Pose {   // what the shim reads of an Eigen::Isometry3d
  double R[9], t[3];
  struct Lin { const double* R; double operator()(int r, int c) const { return R[r * 3 + c]; } };
  struct Tr { const double* t; double operator()(int r) const { return t[r]; } };
  Lin linear() const { return Lin{R}; }
  Tr translation() const { return Tr{t}; }
};

int main() {
  Cloud c1, c2;
  for (int i = 0; i < 300; ++i) c1.points.push_back(Point{0.125f * (float)(i % 20), 0.25f * (float)(i / 20), 0.0625f * (float)((i * 7) % 11)});
  for (int i = 0; i < 130; ++i) c2.points.push_back(Point{0.1875f * (float)(i % 13) + 0.03125f, 0.375f * (float)(i / 13), 0.09375f * (float)((i * 5) % 7)});
  c2.points[17].y = NAN;
  const double c = 0.9950041652780258, s = 0.09983341664682815;   // cos, sin of 0.1 about z
  const Pose rel{{c, -s, 0, s, c, 0, 0, 0, 1}, {0.05, -0.02, 0.01}};
  ps_graph_slam::InformationMatrixCalculator calc;
  const std::array<double, 36> k = calc.calc_information_matrix();
  if (k[0] != 1.0 / 0.0667 || k[35] != 1.0 / 0.0667 || k[1] != 0) { std::printf("constant matrix wrong\n"); return 2; }
  const std::array<double, 36> w = calc.from_score(0.05);
  if (!(w[0] > 0) || !(w[21] > w[0])) { std::printf("information of a score wrong\n"); return 2; }
  if (sslam_device_count() < 1) { std::printf("shim information ok (no GPU: compile/link/host-logic only)\n"); return 0; }
  const double score = ps_graph_slam::InformationMatrixCalculator::calc_fitness_score(c1, c2, rel, 0.04);
  const std::array<double, 36> inf = calc.calc_information_matrix(c1, c2, rel);
  // the plain-array route gives the same bits
  std::vector<float> a, b;
  for (const Point& p : c1.points) { a.push_back(p.x); a.push_back(p.y); a.push_back(p.z); }
  for (const Point& p : c2.points) { b.push_back(p.x); b.push_back(p.y); b.push_back(p.z); }
  double T[12];
  for (int q = 0; q < 9; ++q) T[q] = rel.R[q];
  for (int q = 0; q < 3; ++q) T[9 + q] = rel.t[q];
  const double score2 = ps_graph_slam::InformationMatrixCalculator::calc_fitness_score(a.data(), 300, b.data(), 130, T, 0.04);
  if (score2 != score) { std::printf("array route differs: %.17g %.17g\n", score, score2); return 3; }
  std::printf("shim information ok: score %.17g info", score);
  for (double v : inf) std::printf(" %.17g", v);
  std::printf("\n");
  return 0;
}
