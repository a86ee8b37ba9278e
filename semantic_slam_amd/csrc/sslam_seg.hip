// MI355X-native frontend: point_cloud_segmentation::segmentallPointCloudData
// (reference include/planar_segmentation/point_cloud_segmentation.h:105-181,
//  src/planar_segmentation/plane_segmentation.cpp:24-259) as hand-written HIP for gfx950.
//
// The two PCL calls of the reference (IntegralImageNormalEstimation::compute and
// OrganizedMultiPlaneSegmentation::segmentAndRefine, plane_segmentation.cpp:97-104,136-156) are
// restated kernel by kernel.  Parity rule: labels / inlier sets must be bit-identical with the CPU
// oracle, so every float/double expression keeps PCL's operation order (this file is compiled with
// -ffp-contract=off) and the inherently sequential raster recurrences of PCL (integral-image
// recurrence, two-pass chamfer distance map, two-sweep label refinement) are executed as *skewed
// wavefronts*: lane l of a wave owns image row r0+l and runs two columns behind lane l-1, which
// reproduces the sequential order exactly while 64 rows progress in parallel.  Everything that is
// order-free (crop, depth-change map, per-pixel covariance + eigen solve, comparator evaluation,
// union-find connected components) is one thread per pixel.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "../../include/sslam.h"
#include "map_cloud.hpp"
#include "occupancy_map.hpp"
#include "odometry.hpp"
#include "sslam_common.hpp"
#include "sslam_math.hpp"

namespace sslam {
namespace seg {

constexpr int kMaxRegions = 64;
constexpr int kBandFloats = 30720;  // LDS floats available to a band-staging kernel (120 KiB)

struct BoxMeta {
  int w, h, tlx, tly;
  int pix0;   // offset into the packed per-pixel arrays
  int ii0;    // offset into the packed integral-image arrays ((w+1)*(h+1) per box)
  int box_index, frame;   // frame: which cloud of a batched call the box is cut from
};

struct Region {
  float centroid[3];
  float model[4];
  int inliers, first_inlier, label, contour_n;
  float area;
  int contour_off;   // start of this region's boundary indices in the box's contour arena (-1: not stored)
  int pad0;
  unsigned long long last_key;  // (pass << 60) | (order key << 24) | pixel index
};

struct View {
  int nbox, npix_total, maxpix;
  const BoxMeta* box;
  const unsigned char* cloud;   // the clouds of all frames of the call, cloud_stride bytes apart
  size_t cloud_stride;
  int* overflow;                // [2]: boxes whose candidate / region tables were full (results truncated, reported to the caller)
  int point_step, row_step, ox, oy, oz;
  float* pts;    // [npix*3]
  float* dm;     // [npix]
  float* nrm;    // [npix*4]
  float* pd;     // [npix]
  int* lab;      // [npix] connected-component root (pixel index inside the box) or -1
  int* cnt;      // [npix] pixels per root
  int* l2m;      // [npix] root label -> region index, or -1
  int* code;     // [npix] region index | kOther | -1  (labels as seen by refinement / contour)
  double* ii;    // [nii*10] integral images, one 80-byte record per entry: first order (3), second order (6), finite-point count
  Region* reg;   // [nbox*kMaxRegions]
  int* contour;  // [4*npix] boundary pixel indices, one arena of 4*w*h ints per box at 4*pix0
  int* ccount;   // [nbox] ints used in each arena
  int* nreg;     // [nbox]
  float mdcf, smoothing, ang_thr_cos, dist_thr, max_curv;
  unsigned min_inliers;
  int refine_bh;   // rows per LDS band of k_refine (64: one box per CU, lowest latency; 24: three boxes per CU for calls with many boxes)
};

// ---------------------------------------------------------------------------------------------
// pcl::eigen33 (smallest eigenpair), float, same operation order as oracle/oracle_seg.c
__device__ __forceinline__ void roots2(float b, float c, float r[3]) {
  r[0] = 0.0f;
  float d = b * b - 4.0f * c;
  if (d < 0.0f) d = 0.0f;
  const float sd = sqrtf(d);
  r[2] = 0.5f * (b + sd);
  r[1] = 0.5f * (b - sd);
}
__device__ __forceinline__ void compute_roots(const float m[9], float r[3]) {
  const float m00 = m[0], m01 = m[1], m02 = m[2], m11 = m[4], m12 = m[5], m22 = m[8];
  const float c0 = m00 * m11 * m22 + 2.0f * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01;
  const float c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12;
  const float c2 = m00 + m11 + m22;
  if (fabsf(c0) < 1.1920929e-07f) { roots2(c2, c1, r); return; }
  const float s_inv3 = 1.0f / 3.0f;
  const float s_sqrt3 = sqrtf(3.0f);
  const float c2_over_3 = c2 * s_inv3;
  float a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
  if (a_over_3 > 0.0f) a_over_3 = 0.0f;
  const float half_b = 0.5f * (c0 + c2_over_3 * (2.0f * c2_over_3 * c2_over_3 - c1));
  float q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
  if (q > 0.0f) q = 0.0f;
  const float rho = sqrtf(-a_over_3);
  // trigonometry in double, rounded to float: identical bits on glibc and ocml
  const float theta = (float)atan2((double)sqrtf(-q), (double)half_b) * s_inv3;
  const float cos_theta = (float)cos((double)theta);
  const float sin_theta = (float)sin((double)theta);
  r[0] = c2_over_3 + 2.0f * rho * cos_theta;
  r[1] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
  r[2] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
  float t;
  if (r[0] >= r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
  if (r[1] >= r[2]) {
    t = r[1]; r[1] = r[2]; r[2] = t;
    if (r[0] >= r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
  }
  if (r[0] <= 0.0f) roots2(c2, c1, r);
}
__device__ __forceinline__ void cross3(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void eigen33(const float mat[9], float& eigenvalue, float vec[3]) {
  float scale = 0;
#pragma unroll
  for (int k = 0; k < 9; ++k) { const float a = fabsf(mat[k]); if (a > scale) scale = a; }
  if (scale <= 1.17549435e-38f) scale = 1.0f;
  float s[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) s[k] = mat[k] / scale;
  float r[3];
  compute_roots(s, r);
  eigenvalue = r[0] * scale;
  s[0] -= r[0]; s[4] -= r[0]; s[8] -= r[0];
  float v1[3], v2[3], v3[3];
  cross3(s + 0, s + 3, v1); cross3(s + 0, s + 6, v2); cross3(s + 3, s + 6, v3);
  const float l1 = v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2];
  const float l2 = v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2];
  const float l3 = v3[0] * v3[0] + v3[1] * v3[1] + v3[2] * v3[2];
  float v[3], l;
  if (l1 >= l2 && l1 >= l3) { v[0] = v1[0]; v[1] = v1[1]; v[2] = v1[2]; l = l1; }
  else if (l2 >= l1 && l2 >= l3) { v[0] = v2[0]; v[1] = v2[1]; v[2] = v2[2]; l = l2; }
  else { v[0] = v3[0]; v[1] = v3[1]; v[2] = v3[2]; l = l3; }
  const float n = sqrtf(l);
  vec[0] = v[0] / n; vec[1] = v[1] / n; vec[2] = v[2] / n;
}

// ---------------------------------------------------------------------------------------------
// crop (plane_segmentation.cpp:24-82): box pixels of the organised cloud -> packed xyz
__global__ __launch_bounds__(256) void k_crop(View V) {
  const BoxMeta b = V.box[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= b.w * b.h) return;
  const int v = i / b.w, u = i - v * b.w;
  const size_t pos = (size_t)b.frame * V.cloud_stride + (size_t)(b.tly + v) * V.row_step + (size_t)(b.tlx + u) * V.point_step;
  float x, y, z;
  memcpy(&x, V.cloud + pos + V.ox, 4); memcpy(&y, V.cloud + pos + V.oy, 4); memcpy(&z, V.cloud + pos + V.oz, 4);
  float* o = V.pts + ((size_t)b.pix0 + i) * 3;
  o[0] = x; o[1] = y; o[2] = z;
}

// depth-change map in gather form + distance-map initialisation
__device__ __forceinline__ bool dc_right(const float* pts, int w, int r, int c, float f) {
  const float d = pts[((size_t)r * w + c) * 3 + 2], dR = pts[((size_t)r * w + c + 1) * 3 + 2];
  const float thr = f * (fabsf(d) + 1.0f) * 2.0f;
  return fabsf(d - dR) > thr || !isfinite(d) || !isfinite(dR);
}
__device__ __forceinline__ bool dc_down(const float* pts, int w, int r, int c, float f) {
  const float d = pts[((size_t)r * w + c) * 3 + 2], dD = pts[((size_t)(r + 1) * w + c) * 3 + 2];
  const float thr = f * (fabsf(d) + 1.0f) * 2.0f;
  return fabsf(d - dD) > thr || !isfinite(d) || !isfinite(dD);
}
__global__ __launch_bounds__(256) void k_depth_change(View V) {
  const BoxMeta b = V.box[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int w = b.w, h = b.h;
  if (i >= w * h) return;
  const int r = i / w, c = i - r * w;
  const float* pts = V.pts + (size_t)b.pix0 * 3;
  bool zero = false;
  if (r < h - 1 && c < w - 1) zero = dc_right(pts, w, r, c, V.mdcf) || dc_down(pts, w, r, c, V.mdcf);
  if (!zero && c >= 1 && r < h - 1) zero = dc_right(pts, w, r, c - 1, V.mdcf);
  if (!zero && r >= 1 && c < w - 1) zero = dc_down(pts, w, r - 1, c, V.mdcf);
  V.dm[(size_t)b.pix0 + i] = zero ? 0.0f : (float)(w + h);
  // normals default to NaN; labels to "invalid"
  float* nn = V.nrm + ((size_t)b.pix0 + i) * 4;
  const float qnan = __int_as_float(0x7fc00000);
  nn[0] = qnan; nn[1] = qnan; nn[2] = qnan; nn[3] = qnan;
}

// two-pass chamfer distance map: skewed wavefront over rows, band staged in LDS with the image's
// own row stride (so PCL's wrap-around reads prev[w] == cur[0], next[-1] == cur[w-1] come for free)
__global__ __launch_bounds__(256) void k_distance_map(View V) {
  extern __shared__ float band[];
  const BoxMeta b = V.box[blockIdx.x];
  const int w = b.w, h = b.h;
  float* dm = V.dm + b.pix0;
  const int BH = min(64, kBandFloats / w - 1);
  // ---- forward pass: rows 1 .. h-1
  for (int r0 = 1; r0 < h; r0 += BH) {
    const int nr = min(BH, h - r0);
    for (int k = threadIdx.x; k < (nr + 1) * w; k += 256) band[k] = dm[(size_t)(r0 - 1) * w + k];
    __syncthreads();
    if (threadIdx.x < 64) {
      const int l = threadIdx.x;
      const int steps = (w - 1) + 2 * (nr - 1);
      for (int t = 0; t < steps; ++t) {
        const int c = t - 2 * l + 1;
        if (l < nr && c >= 1 && c < w) {
          const float* prev = band + l * w;
          float* cur = band + (l + 1) * w;
          const float upLeft = prev[c - 1] + 1.4f, up = prev[c] + 1.0f, upRight = prev[c + 1] + 1.4f, left = cur[c - 1] + 1.0f;
          const float center = cur[c];
          const float m = fminf(fminf(upLeft, up), fminf(left, upRight));
          if (m < center) cur[c] = m;
        }
      }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nr * w; k += 256) dm[(size_t)r0 * w + k] = band[w + k];
    __syncthreads();
  }
  // ---- backward pass: rows h-2 .. 0
  for (int rhi = h - 2; rhi >= 0; rhi -= BH) {
    const int nr = min(BH, rhi + 1);
    const int rlo = rhi - nr + 1;
    for (int k = threadIdx.x; k < (nr + 1) * w; k += 256) band[k] = dm[(size_t)rlo * w + k];
    __syncthreads();
    if (threadIdx.x < 64) {
      const int l = threadIdx.x;  // lane l owns row rhi - l = band row (nr - 1 - l)
      const int steps = (w - 1) + 2 * (nr - 1);
      for (int t = 0; t < steps; ++t) {
        const int c = (w - 2) - (t - 2 * l);
        if (l < nr && c >= 0 && c <= w - 2) {
          float* cur = band + (nr - 1 - l) * w;
          const float* next = cur + w;
          // (row 0, column 0 would read next[-1] = cur[w-1]; for band row 0 that is band[w-1]: in range)
          const float lowerLeft = next[c - 1] + 1.4f, lower = next[c] + 1.0f, lowerRight = next[c + 1] + 1.4f, right = cur[c + 1] + 1.0f;
          const float center = cur[c];
          const float m = fminf(fminf(lowerLeft, lower), fminf(right, lowerRight));
          if (m < center) cur[c] = m;
        }
      }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nr * w; k += 256) dm[(size_t)rlo * w + k] = band[k];
    __syncthreads();
  }
}

// integral images (IntegralImage2D<float,3>::computeIntegralImages, second order on).  Lane l of a wave owns row r0+l, two columns
// behind lane l-1; the previous row's running values arrive by wave shuffle.  Recurrence and operation order are PCL's:
// cur[c+1] = prev[c+1] + cur[c] - prev[c] (+ element).  The ten running sums (x y z | xx xy xz | yy yz | zz count) are independent of
// one another, so the four waves of the workgroup each carry two or three of them over the same rows: a step is bound by one wave's
// instruction issue, and no barrier is needed between the waves.  One 80-byte record per entry: [x y z xx xy xz yy yz zz count].
struct alignas(16) IiPair { double a, b; };
template <int Q>
__device__ __forceinline__ float ii_elem(float ex, float ey, float ez) {
  return Q == 0 ? ex : Q == 1 ? ey : Q == 2 ? ez : Q == 3 ? ex * ex : Q == 4 ? ex * ey : Q == 5 ? ex * ez : Q == 6 ? ey * ey : Q == 7 ? ey * ez : Q == 8 ? ez * ez : 1.0f;
}
template <int C0, int NC>
__device__ __forceinline__ void ii_store(double* e, const double (&v)[NC]) {   // e = record + C0; 16-byte stores where the pair is aligned
  if (NC == 2) { *reinterpret_cast<IiPair*>(e) = IiPair{v[0], v[1]}; }
  else if (C0 % 2 == 0) { *reinterpret_cast<IiPair*>(e) = IiPair{v[0], v[1]}; e[2] = v[NC - 1]; }
  else { e[0] = v[0]; *reinterpret_cast<IiPair*>(e + 1) = IiPair{v[1], v[NC - 1]}; }
}
template <int C0, int NC>
__device__ __forceinline__ void integral_wave(const float* bpts, const double* prevrow, double* rec, int w, int nr, int r0, int l) {
  const int W1 = w + 1, r = r0 + l;
  double cur[NC], h1[NC], h2[NC], p0[NC];   // cur[c] of the running column; own outputs one / two steps ago; prev[c]
#pragma unroll
  for (int q = 0; q < NC; ++q) { cur[q] = 0; h1[q] = 0; h2[q] = 0; p0[q] = 0; }
  const int steps = w + 2 * (nr - 1);
  for (int t = 0; t < steps; ++t) {
    const int c = t - 2 * l;
    // prev[c+1]: lane l-1's output two steps ago; lane 0 reads the staged last row of the previous band
    double p1[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) p1[q] = __shfl_up(h2[q], 1, 64);
    const bool active = l < nr && c >= 0 && c < w;
    if (l == 0 && active) {
#pragma unroll
      for (int q = 0; q < NC; ++q) p1[q] = prevrow[(c + 1) * 10 + C0 + q];
    }
    double out[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) out[q] = h1[q];
    if (active) {
#pragma unroll
      for (int q = 0; q < NC; ++q) out[q] = p1[q] + cur[q] - p0[q];
      const float* ep = bpts + ((size_t)l * w + c) * 3;
      const float ex = ep[0], ey = ep[1], ez = ep[2];
      if (isfinite(ex + ey + ez)) {
        out[0] += (double)ii_elem<C0>(ex, ey, ez);
        out[1] += (double)ii_elem<C0 + 1>(ex, ey, ez);
        if (NC == 3) out[NC - 1] += (double)ii_elem<C0 + NC - 1>(ex, ey, ez);
      }
      const size_t o = (size_t)(r + 1) * W1 + (c + 1);
      ii_store<C0, NC>(rec + o * 10 + C0, out);
      if (c == 0) {  // integral column 0 of this row is zero
        const double zero[NC] = {};
        ii_store<C0, NC>(rec + (size_t)(r + 1) * W1 * 10 + C0, zero);
      }
#pragma unroll
      for (int q = 0; q < NC; ++q) { cur[q] = out[q]; p0[q] = p1[q]; }
    }
    // shift the output history (every lane, every step: the shuffle above reads h2)
#pragma unroll
    for (int q = 0; q < NC; ++q) { h2[q] = h1[q]; h1[q] = out[q]; }
  }
}
__global__ __launch_bounds__(256) void k_integral(View V, int band_rows) {
  extern __shared__ double prevrow[];  // (w+1) x 10 doubles: last row of the previous band; then the band's points (floats)
  const BoxMeta b = V.box[blockIdx.x];
  const int w = b.w, h = b.h, W1 = w + 1;
  const float* pts = V.pts + (size_t)b.pix0 * 3;
  float* bpts = reinterpret_cast<float*>(prevrow + (size_t)W1 * 10);
  double* rec = V.ii + (size_t)b.ii0 * 10;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // row 0 of the integral images is zero
  for (int k = tid; k < W1 * 10; k += 256) { rec[k] = 0; prevrow[k] = 0; }
  __syncthreads();
  for (int r0 = 0; r0 < h; r0 += band_rows) {
    const int nr = min(band_rows, h - r0);
    for (int k = tid; k < nr * w * 3; k += 256) bpts[k] = pts[(size_t)r0 * w * 3 + k];   // coalesced
    __syncthreads();
    if (wave == 0) integral_wave<0, 3>(bpts, prevrow, rec, w, nr, r0, lane);
    else if (wave == 1) integral_wave<3, 3>(bpts, prevrow, rec, w, nr, r0, lane);
    else if (wave == 2) integral_wave<6, 2>(bpts, prevrow, rec, w, nr, r0, lane);
    else integral_wave<8, 2>(bpts, prevrow, rec, w, nr, r0, lane);
    // stage the last row of this band for the next band's lane 0
    __syncthreads();
    if (r0 + band_rows < h) {
      const double* src = rec + (size_t)(r0 + band_rows) * W1 * 10;     // same record layout as the carry row
      for (int k = tid; k < W1 * 10; k += 256) prevrow[k] = src[k];
    }
    __syncthreads();
  }
}

// per-pixel normal: IntegralImageNormalEstimation::computePointNormal (COVARIANCE_MATRIX),
// BORDER_POLICY_IGNORE, fixed smoothing size
__global__ __launch_bounds__(256) void k_normals(View V) {
  const BoxMeta b = V.box[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int w = b.w, h = b.h, W1 = w + 1;
  if (i >= w * h) return;
  const int r = i / w, c = i - r * w;
  const int border = (int)V.smoothing;
  if (r < border || r >= h - border || c < border || c >= w - border) return;
  const float* pts = V.pts + (size_t)b.pix0 * 3;
  const float depth = pts[(size_t)i * 3 + 2];
  if (!isfinite(depth)) return;
  const float smoothing = fminf(V.dm[(size_t)b.pix0 + i], V.smoothing);
  if (!(smoothing > 2.0f)) return;
  const int rw = (int)smoothing, rh = (int)smoothing;
  const int sx = c - rw / 2, sy = r - rh / 2;
  const size_t ul = (size_t)sy * W1 + sx, ur = ul + rw, ll = (size_t)(sy + rh) * W1 + sx, lr = ll + rw;
  const double* ii = V.ii + (size_t)b.ii0 * 10;
  const unsigned count = (unsigned)ii[lr * 10 + 9] + (unsigned)ii[ul * 10 + 9] - (unsigned)ii[ur * 10 + 9] - (unsigned)ii[ll * 10 + 9];
  if (count == 0) return;
  float cen[3], sov[6], cov[9];
#pragma unroll
  for (int k = 0; k < 3; ++k) cen[k] = (float)(ii[lr * 10 + k] + ii[ul * 10 + k] - ii[ur * 10 + k] - ii[ll * 10 + k]);
#pragma unroll
  for (int k = 0; k < 6; ++k) sov[k] = (float)(ii[lr * 10 + 3 + k] + ii[ul * 10 + 3 + k] - ii[ur * 10 + 3 + k] - ii[ll * 10 + 3 + k]);
  cov[0] = sov[0]; cov[1] = cov[3] = sov[1]; cov[2] = cov[6] = sov[2]; cov[4] = sov[3]; cov[5] = cov[7] = sov[4]; cov[8] = sov[5];
  const float fc = (float)count;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int bb = 0; bb < 3; ++bb) cov[a * 3 + bb] -= (cen[a] * cen[bb]) / fc;
  float ev, v[3];
  eigen33(cov, ev, v);
  const float vx = 0.0f - pts[(size_t)i * 3 + 0], vy = 0.0f - pts[(size_t)i * 3 + 1], vz = 0.0f - pts[(size_t)i * 3 + 2];
  const float ct = vx * v[0] + vy * v[1] + vz * v[2];
  if (ct < 0) { v[0] *= -1; v[1] *= -1; v[2] *= -1; }
  float* nn = V.nrm + ((size_t)b.pix0 + i) * 4;
  nn[0] = v[0]; nn[1] = v[1]; nn[2] = v[2];
  nn[3] = ev > 0.0f ? fabsf(ev / (cov[0] + cov[4] + cov[8])) : 0.0f;
}

// ---------------------------------------------------------------------------------------------
// OrganizedConnectedComponentSegmentation with the PlaneCoefficientComparator (depth dependent)
__global__ __launch_bounds__(256) void k_cc_init(View V) {
  const BoxMeta b = V.box[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= b.w * b.h) return;
  const size_t g = (size_t)b.pix0 + i;
  const float* p = V.pts + g * 3;
  const float* n = V.nrm + g * 4;
  V.pd[g] = p[0] * n[0] + p[1] * n[1] + p[2] * n[2];
  V.lab[g] = isfinite(p[0]) ? i : -1;
  V.cnt[g] = 0;
  V.l2m[g] = -1;
}
__device__ __forceinline__ bool coeff_compare(const View& V, size_t g1, size_t g2) {
  const float z = V.pts[g1 * 3 + 2];
  const float thr = V.dist_thr * (z * z);
  const float* a = V.nrm + g1 * 4;
  const float* b = V.nrm + g2 * 4;
  const float dot = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
  return (fabsf(V.pd[g1] - V.pd[g2]) < thr) && (dot > V.ang_thr_cos);
}
__device__ __forceinline__ int uf_find(int* L, int i) {
  int p = L[i];
  while (p != i) { i = p; p = L[i]; }
  return i;
}
__device__ __forceinline__ void uf_union(int* L, int a, int b) {
  while (true) {
    a = uf_find(L, a); b = uf_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }   // attach the larger root to the smaller one
    const int old = atomicMin(&L[a], b);
    if (old == a) return;
    a = old;
  }
}
__global__ __launch_bounds__(256) void k_cc_merge(View V) {
  const BoxMeta b = V.box[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int w = b.w;
  if (i >= w * b.h) return;
  int* L = V.lab + b.pix0;
  if (L[i] < 0) return;
  const int r = i / w, c = i - r * w;
  const size_t g = (size_t)b.pix0 + i;
  if (c > 0 && L[i - 1] >= 0 && coeff_compare(V, g, g - 1)) uf_union(L, i, i - 1);
  if (r > 0 && L[i - w] >= 0 && coeff_compare(V, g, g - w)) uf_union(L, i, i - w);
}
__global__ __launch_bounds__(256) void k_cc_flatten(View V) {
  const BoxMeta b = V.box[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= b.w * b.h) return;
  int* L = V.lab + b.pix0;
  if (L[i] < 0) return;
  const int root = uf_find(L, i);
  atomicAdd(&V.cnt[b.pix0 + root], 1);
  // roots only ever point at themselves, so writing the flattened parent is race-free
  if (root != i) L[i] = root;
}
__global__ __launch_bounds__(256) void k_cc_flatten2(View V) {  // second hop: every pixel points at its root
  const BoxMeta b = V.box[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= b.w * b.h) return;
  int* L = V.lab + b.pix0;
  if (L[i] >= 0) L[i] = uf_find(L, i);
}

// The four kernels above as ONE workgroup per box with the union-find forest in LDS (boxes of <= kCcLdsMax pixels; the YOLO boxes of
// the reference are a few thousand pixels).  Roots are the smallest pixel index of a component whatever the order of the unions, so
// labels and counts are those of the global-memory kernels; the comparator's plane distance p.n is recomputed for the neighbour
// (same expression, no contraction) instead of being parked in HBM.  LDS: 4 bytes per pixel -> three 12k-pixel boxes per CU.
constexpr int kCcLdsMax = 16384;
__device__ __forceinline__ bool coeff_compare_direct(const View& V, size_t g1, size_t g2) {
  const float* p1 = V.pts + g1 * 3;
  const float* p2 = V.pts + g2 * 3;
  const float* a = V.nrm + g1 * 4;
  const float* b = V.nrm + g2 * 4;
  const float pd1 = p1[0] * a[0] + p1[1] * a[1] + p1[2] * a[2];
  const float pd2 = p2[0] * b[0] + p2[1] * b[1] + p2[2] * b[2];
  const float z = p1[2];
  const float thr = V.dist_thr * (z * z);
  const float dot = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
  return (fabsf(pd1 - pd2) < thr) && (dot > V.ang_thr_cos);
}
__global__ __launch_bounds__(1024) void k_cc_lds(View V) {
  extern __shared__ int Ls[];
  constexpr int NT = 1024, PER = kCcLdsMax / NT;
  const BoxMeta b = V.box[blockIdx.x];
  const int w = b.w, n = w * b.h, tid = threadIdx.x;
  for (int i = tid; i < n; i += NT) {
    const size_t g = (size_t)b.pix0 + i;
    Ls[i] = isfinite(V.pts[g * 3]) ? i : -1;
    V.l2m[g] = -1;
  }
  __syncthreads();
  for (int i = tid; i < n; i += NT) {
    if (Ls[i] < 0) continue;
    const int r = i / w, c = i - r * w;
    const size_t g = (size_t)b.pix0 + i;
    if (c > 0 && Ls[i - 1] >= 0 && coeff_compare_direct(V, g, g - 1)) uf_union(Ls, i, i - 1);
    if (r > 0 && Ls[i - w] >= 0 && coeff_compare_direct(V, g, g - w)) uf_union(Ls, i, i - w);
  }
  __syncthreads();
  int root[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = tid + k * NT;
    root[k] = (i < n && Ls[i] >= 0) ? uf_find(Ls, i) : -1;
  }
  __syncthreads();   // every find is done: the forest may go
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = tid + k * NT;
    if (i < n) { V.lab[(size_t)b.pix0 + i] = root[k]; Ls[i] = 0; }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PER; ++k) if (root[k] >= 0) atomicAdd(&Ls[root[k]], 1);
  __syncthreads();
  for (int i = tid; i < n; i += NT) V.cnt[(size_t)b.pix0 + i] = Ls[i];
}

// per-label plane fit (OrganizedMultiPlaneSegmentation::segment): labels with more than
// min_inliers pixels; PCL accumulates the 9 float sums in index (raster) order, so the additions stay
// a serial chain, but everything around them is parallel: candidate roots are found by all threads,
// each candidate gets a wave, pixels are loaded 64 at a time (coalesced), the 9 products are formed
// lane-parallel and parked in LDS, and lanes 0..8 each run one component's chain over the chunk.
// NT = 1024 (16 candidates at a time) for a call with few boxes; NT = 256 when a call brings more boxes than the chip has CUs: a box
// rarely has more than four candidate labels, and four times as many boxes are resident.
constexpr int kMaxCand = 64;
template <int NT>
__global__ __launch_bounds__(NT) void k_regions(View V) {
  constexpr int NW = NT / 64;
  __shared__ int cand[kMaxCand];
  __shared__ int ncand;
  __shared__ int accepted[kMaxCand];
  __shared__ float prod[NW][64][9];
  __shared__ Region regs[kMaxCand];
  const BoxMeta b = V.box[blockIdx.x];
  const int n = b.w * b.h;
  const int* L = V.lab + b.pix0;
  const int* cnt = V.cnt + b.pix0;
  const float* pts = V.pts + (size_t)b.pix0 * 3;
  if (threadIdx.x == 0) ncand = 0;
  if (threadIdx.x < kMaxCand) accepted[threadIdx.x] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += NT)
    if (L[i] == i && (unsigned)cnt[i] > V.min_inliers) { const int k = atomicAdd(&ncand, 1); if (k < kMaxCand) cand[k] = i; }
  __syncthreads();
  if (ncand > kMaxCand) {
    // Full table: which 64 roots the atomic counter let in depends on the arrival order of the threads.  Keep the 64 LOWEST roots
    // instead -- PCL hands its labels out in root order and stops accepting after 64 regions, so this is the set the reference fits
    // first.  One wave walks the pixels in ascending chunks of 64 and ranks the roots of a chunk by ballot; taken only on overflow.
    if (threadIdx.x < 64) {
      int taken = 0;
      for (int i0 = 0; i0 < n && taken < kMaxCand; i0 += 64) {
        const int i = i0 + (int)threadIdx.x;
        const bool m = i < n && L[i] == i && (unsigned)cnt[i] > V.min_inliers;
        const unsigned long long mask = __ballot(m);
        const int rank = taken + __popcll(mask & ((1ull << threadIdx.x) - 1ull));
        if (m && rank < kMaxCand) cand[rank] = i;
        taken += __popcll(mask);
      }
    }
    __syncthreads();
  }
  const int nc = min(ncand, kMaxCand);
  if (threadIdx.x == 0) {  // order by root pixel index = PCL's label order (insertion sort, short list)
    for (int a = 1; a < nc; ++a) { const int v = cand[a]; int q = a - 1; while (q >= 0 && cand[q] > v) { cand[q + 1] = cand[q]; --q; } cand[q + 1] = v; }
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int k = wave; k < nc; k += NW) {
    const int label = cand[k];
    float acc = 0;            // lanes 0..8: component `lane`
    int first = -1, last = -1;
    // the labels and points of the next FOUR chunks travel while a chunk's serial additions run: with one chunk ahead (round 3) the loop was one
    // L2 round trip per 64 pixels long -- 90 % of the kernel's wave cycles parked (profiles/r6_pmc_frontend.json)
    constexpr int PF = 4;
    int lq[PF];
    float xq[PF], yq[PF], zq[PF];
#pragma unroll
    for (int c = 0; c < PF; ++c) {
      const int j = 64 * c + lane;
      lq[c] = j < n ? L[j] : -2; xq[c] = yq[c] = zq[c] = 0;
      if (j < n) { xq[c] = pts[(size_t)j * 3]; yq[c] = pts[(size_t)j * 3 + 1]; zq[c] = pts[(size_t)j * 3 + 2]; }
    }
    for (int i00 = 0; i00 < n; i00 += 64 * PF) {
#pragma unroll
      for (int c = 0; c < PF; ++c) {
        const int i0 = i00 + 64 * c;
        const int i = i0 + lane;
        const bool m = i < n && lq[c] == label;
        const float x = xq[c], y = yq[c], z = zq[c];
        {
          const int j = i + 64 * PF;
          lq[c] = j < n ? L[j] : -2;
          if (j < n) { xq[c] = pts[(size_t)j * 3]; yq[c] = pts[(size_t)j * 3 + 1]; zq[c] = pts[(size_t)j * 3 + 2]; }
        }
        if (m) {
          float* p = prod[wave][lane];
          p[0] = x * x; p[1] = x * y; p[2] = x * z; p[3] = y * y; p[4] = y * z; p[5] = z * z; p[6] = x; p[7] = y; p[8] = z;
        }
        const unsigned long long mask = __ballot(m);
        if (mask) {
          if (first < 0) first = i0 + __ffsll((long long)mask) - 1;
          last = i0 + 63 - __clzll((long long)mask);
          // the additions are a serial chain in pixel order (PCL's), the LDS reads are not: eight products are fetched together,
          // then added under the (wave-uniform) inlier bits
          if (lane < 9) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const unsigned bits = (unsigned)(mask >> (8 * j)) & 0xffu;
              if (bits) {
                float v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = prod[wave][8 * j + q][lane];
#pragma unroll
                for (int q = 0; q < 8; ++q) if (bits & (1u << q)) acc += v[q];
              }
            }
          }
        }
      }
    }
    float a[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) a[q] = __shfl(acc, q, 64);
    if (lane == 0) {
      const float cntf = (float)cnt[label];
#pragma unroll
      for (int q = 0; q < 9; ++q) a[q] = a[q] / cntf;
      float cov[9];
      cov[0] = a[0] - a[6] * a[6]; cov[1] = a[1] - a[6] * a[7]; cov[2] = a[2] - a[6] * a[8];
      cov[4] = a[3] - a[7] * a[7]; cov[5] = a[4] - a[7] * a[8]; cov[8] = a[5] - a[8] * a[8];
      cov[3] = cov[1]; cov[6] = cov[2]; cov[7] = cov[5];
      float ev, v[3];
      eigen33(cov, ev, v);
      float p[4] = {v[0], v[1], v[2], 0};
      p[3] = -1 * (p[0] * a[6] + p[1] * a[7] + p[2] * a[8]);
      const float ct = (0.0f - a[6]) * p[0] + (0.0f - a[7]) * p[1] + (0.0f - a[8]) * p[2];
      if (ct < 0) {
        p[0] *= -1; p[1] *= -1; p[2] *= -1;
        p[3] = -1 * (p[0] * a[6] + p[1] * a[7] + p[2] * a[8]);
      }
      const float es = cov[0] + cov[4] + cov[8];
      const float curv = es != 0 ? fabsf(ev / es) : 0;
      Region R;
      R.centroid[0] = a[6]; R.centroid[1] = a[7]; R.centroid[2] = a[8];
      R.model[0] = p[0]; R.model[1] = p[1]; R.model[2] = p[2]; R.model[3] = p[3];
      R.inliers = cnt[label]; R.first_inlier = first; R.label = label; R.contour_n = 0; R.area = 0;
      R.last_key = (unsigned long long)(unsigned)last;
      regs[k] = R;
      accepted[k] = curv < V.max_curv ? 1 : 0;
    }
  }
  __syncthreads();
  if (threadIdx.x < nc && accepted[threadIdx.x]) {
    int idx = 0;
    for (int q = 0; q < (int)threadIdx.x; ++q) idx += accepted[q];
    if (idx < kMaxRegions) {
      V.reg[(size_t)blockIdx.x * kMaxRegions + idx] = regs[threadIdx.x];
      V.l2m[b.pix0 + regs[threadIdx.x].label] = idx;
    }
  }
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int q = 0; q < nc; ++q) tot += accepted[q];
    V.nreg[blockIdx.x] = min(tot, kMaxRegions);
    if (ncand > kMaxCand) atomicAdd(&V.overflow[0], 1);
    if (tot > kMaxRegions) atomicAdd(&V.overflow[1], 1);   // cannot fire while kMaxRegions == kMaxCand (tot <= nc); kept for the ABI's third counter
  }
}

// labels -> compact codes for refinement / contour / the label image:
//   region index (0..63) for pixels of an accepted plane, kOther for any other valid pixel, -1 invalid
constexpr int kOther = 1000;
__global__ __launch_bounds__(256) void k_relabel(View V) {
  const BoxMeta b = V.box[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= b.w * b.h) return;
  const int l = V.lab[b.pix0 + i];
  V.code[b.pix0 + i] = l < 0 ? -1 : (V.l2m[b.pix0 + l] >= 0 ? V.l2m[b.pix0 + l] : kOther);
}

// OrganizedMultiPlaneSegmentation::refine: two raster sweeps with the PlaneRefinementComparator,
// executed as skewed wavefronts over a label band staged in LDS (image row stride preserved, so the
// second sweep's colIdx-1 read at column 0 lands on the previous row's last pixel as in PCL).
// PlaneRefinementComparator::compare; p1 / p2 point at the xyz of the current / neighbour pixel (LDS band)
__device__ __forceinline__ bool refine_compare(float dist_thr, const float* models, int cl, int nl, const float* p1, const float* p2) {
  if (!(cl < kMaxRegions && nl >= kMaxRegions)) return false;   // grow[current] && !grow[next]
  const float* m = models + cl * 4;
  const double d = fabs((double)(m[0] * p2[0] + m[1] * p2[1] + m[2] * p2[2] + m[3]));
  const float z = p1[2];
  const float t = dist_thr * (z * z);
  return d < (double)t;
}
__device__ __forceinline__ void refine_record(const View& V, int slot, int model_idx, unsigned long long pass, unsigned long long key, int target) {
  Region* R = &V.reg[(size_t)slot * kMaxRegions + model_idx];
  atomicAdd(&R->inliers, 1);
  atomicMax(&R->last_key, (pass << 60) | (key << 24) | (unsigned long long)target);
}
__global__ __launch_bounds__(256) void k_refine(View V) {
  extern __shared__ int lband[];
  __shared__ float models[kMaxRegions * 4];
  const BoxMeta b = V.box[blockIdx.x];
  const int slot = blockIdx.x;
  const int nregs = V.nreg[slot];
  if (nregs == 0) return;
  for (int k = threadIdx.x; k < nregs * 4; k += 256) models[k] = V.reg[(size_t)slot * kMaxRegions + (k >> 2)].model[k & 3];
  const int w = b.w, h = b.h;
  int* L = V.code + b.pix0;
  const float* gp = V.pts + (size_t)b.pix0 * 3;
  const int BH = min(V.refine_bh, kBandFloats / (4 * w) - 1);     // labels (1 word) + xyz (3 words) per staged pixel
  float* pband = reinterpret_cast<float*>(lband + (BH + 1) * w);
  const float dthr = V.dist_thr;
  __syncthreads();
  // ---- sweep 1: top-down, left-right; checks right then lower neighbour
  for (int r0 = 0; r0 < h - 1; r0 += BH) {
    const int nr = min(BH, h - 1 - r0);
    for (int k = threadIdx.x; k < (nr + 1) * w; k += 256) lband[k] = L[(size_t)r0 * w + k];
    for (int k = threadIdx.x; k < (nr + 1) * w * 3; k += 256) pband[k] = gp[(size_t)r0 * w * 3 + k];
    __syncthreads();
    if (threadIdx.x < 64) {
      // One step = one pixel of this lane's row.  Only the two neighbour labels have to be read after the previous step's writes; the
      // lane's own label is carried in a register (the row above wrote it at least one step before it was read as `rl`), and the
      // points / the plane model of the NEXT step are fetched while this step's labels are on their way.
      const int l = threadIdx.x;
      const int steps = (w - 1) + 2 * (nr - 1);
      const bool rowok = l < nr;
      int* cur = lband + (rowok ? l : 0) * w;
      const float* prow = pband + (size_t)(rowok ? l : 0) * w * 3;
      const int r = r0 + l;
      int cl = -1;
      float z = 0, m0 = 0, m1 = 0, m2 = 0, m3 = 0, pr0 = 0, pr1 = 0, pr2 = 0, pd0 = 0, pd1 = 0, pd2 = 0;
      for (int t = 0; t < steps; ++t) {
        const int c = t - 2 * l;
        const bool act = rowok && c >= 0 && c < w - 1;
        if (act && c == 0) {   // first pixel of the row: nothing carried yet
          cl = cur[0];
          z = prow[2];
          pr0 = prow[3]; pr1 = prow[4]; pr2 = prow[5];
          pd0 = prow[3 * w]; pd1 = prow[3 * w + 1]; pd2 = prow[3 * w + 2];
          const float* m = models + ((cl >= 0 && cl < kMaxRegions) ? cl : 0) * 4;
          m0 = m[0]; m1 = m[1]; m2 = m[2]; m3 = m[3];
        }
        const int cc = act ? c : 0;
        const int rl = cur[cc + 1], ll = cur[w + cc];
        const int cn = min(cc + 1, w - 2);                     // next step's pixel: its right and lower neighbours
        const float* qn = prow + (size_t)(cn + 1) * 3;
        const float* qd = prow + (size_t)(w + cn) * 3;
        const float nr0 = qn[0], nr1 = qn[1], nr2 = qn[2], nd0 = qd[0], nd1 = qd[1], nd2 = qd[2];
        if (act) {
          // PlaneRefinementComparator::compare twice (right, lower): grow[current] && !grow[next] && distance of the next point to the
          // current label's plane < threshold * z^2 of the current point; the lower check only runs when the right label is valid
          const bool ok = cl >= 0 && rl >= 0 && cl < kMaxRegions;
          const float thr = dthr * (z * z);
          const double d1 = fabs((double)(m0 * pr0 + m1 * pr1 + m2 * pr2 + m3));
          const double d2 = fabs((double)(m0 * pd0 + m1 * pd1 + m2 * pd2 + m3));
          const bool c1 = ok && rl >= kMaxRegions && d1 < (double)thr;
          const bool c2 = ok && ll >= kMaxRegions && d2 < (double)thr;
          if (c1) {
            cur[c + 1] = cl;
            refine_record(V, slot, cl, 1ull, (unsigned long long)(r * w + c) * 2ull, r * w + c + 1);
          }
          if (c2) {
            cur[w + c] = cl;
            refine_record(V, slot, cl, 1ull, (unsigned long long)(r * w + c) * 2ull + 1ull, (r + 1) * w + c);
          }
          cl = c1 ? cl : rl;
          z = pr2;
          pr0 = nr0; pr1 = nr1; pr2 = nr2; pd0 = nd0; pd1 = nd1; pd2 = nd2;
          const float* m = models + ((cl >= 0 && cl < kMaxRegions) ? cl : 0) * 4;
          m0 = m[0]; m1 = m[1]; m2 = m[2]; m3 = m[3];
        }
      }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < (nr + 1) * w; k += 256) L[(size_t)r0 * w + k] = lband[k];
    __syncthreads();
  }
  // ---- sweep 2: bottom-up, right-left; checks left then upper neighbour
  for (int rhi = h - 1; rhi >= 1; rhi -= BH) {
    const int nr = min(BH, rhi);
    const int rlo = rhi - nr;  // staged rows rlo .. rhi (rlo is the upper halo of the topmost processed row)
    for (int k = threadIdx.x; k < (nr + 1) * w; k += 256) lband[k] = L[(size_t)rlo * w + k];
    for (int k = threadIdx.x; k < (nr + 1) * w * 3; k += 256) pband[k] = gp[(size_t)rlo * w * 3 + k];
    __syncthreads();
    if (threadIdx.x < 64) {
      const int l = threadIdx.x;  // lane l owns row rhi - l; same register-carried form as sweep 1, mirrored
      const int steps = w + 2 * (nr - 1);
      const bool rowok = l < nr;
      const int r = rhi - (rowok ? l : 0);
      int* cur = lband + (r - rlo) * w;
      const float* prow = pband + (size_t)(r - rlo) * w * 3;
      int cl = -1;
      float z = 0, m0 = 0, m1 = 0, m2 = 0, m3 = 0, pl0 = 0, pl1 = 0, pl2 = 0, pu0 = 0, pu1 = 0, pu2 = 0;
      for (int t = 0; t < steps; ++t) {
        const int c = (w - 1) - (t - 2 * l);
        const bool act = rowok && c >= 0 && c <= w - 1;
        if (act && c == w - 1) {   // first pixel of the row (sweep 2 runs right to left)
          cl = cur[c];
          const float* pc = prow + (size_t)c * 3;
          z = pc[2];
          pl0 = pc[-3]; pl1 = pc[-2]; pl2 = pc[-1];
          pu0 = pc[-3 * w]; pu1 = pc[-3 * w + 1]; pu2 = pc[-3 * w + 2];
          const float* m = models + ((cl >= 0 && cl < kMaxRegions) ? cl : 0) * 4;
          m0 = m[0]; m1 = m[1]; m2 = m[2]; m3 = m[3];
        }
        const int cc = act ? c : 1;
        // column 0 has no left neighbour here (PCL reads the previous row's last pixel): label 0 stands in, unused
        const int lf = cc >= 1 ? cur[cc - 1] : 0;
        const int ul = cur[cc - w];
        const float* ql = prow + (size_t)max(cc - 2, 0) * 3;                       // next step's pixel (c - 1): its left neighbour ...
        const float* qu = prow + (size_t)max(cc - 1, 0) * 3 - (size_t)w * 3;      // ... and its upper neighbour
        const float nl0 = ql[0], nl1 = ql[1], nl2 = ql[2];
        const float nu0 = qu[0], nu1 = qu[1], nu2 = qu[2];
        if (act) {
          const bool ok = cl >= 0 && lf >= 0 && cl < kMaxRegions;
          const float thr = dthr * (z * z);
          const double d1 = fabs((double)(m0 * pl0 + m1 * pl1 + m2 * pl2 + m3));
          const double d2 = fabs((double)(m0 * pu0 + m1 * pu1 + m2 * pu2 + m3));
          const bool c1 = ok && c >= 1 && lf >= kMaxRegions && d1 < (double)thr;
          const bool c2 = ok && ul >= kMaxRegions && d2 < (double)thr;
          const unsigned long long key = (unsigned long long)((h - 1 - r) * w + (w - 1 - c)) * 2ull;
          if (c1) {
            cur[c - 1] = cl;
            refine_record(V, slot, cl, 2ull, key, r * w + c - 1);
          }
          if (c2) {
            cur[c - w] = cl;
            refine_record(V, slot, cl, 2ull, key + 1ull, (r - 1) * w + c);
          }
          cl = c1 ? cl : lf;
          z = pl2;
          pl0 = nl0; pl1 = nl1; pl2 = nl2; pu0 = nu0; pu1 = nu1; pu2 = nu2;
          const float* m = models + ((cl >= 0 && cl < kMaxRegions) ? cl : 0) * 4;
          m0 = m[0]; m1 = m[1]; m2 = m[2]; m3 = m[3];
        }
      }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < (nr + 1) * w; k += 256) L[(size_t)rlo * w + k] = lband[k];
    __syncthreads();
  }
}

// The same two sweeps for boxes whose label image fits LDS (<= kCcLdsMax pixels), as a fixed-point iteration instead of a wavefront.
// A pixel is only ever written while it still carries kOther, and only by the two neighbours the raster order visits before it (sweep 1:
// the upper one first, then the left one; sweep 2: the lower one first, then the right one), each with the label it ends the sweep with.
// So the result of a sweep is the unique solution of   label(T) = F(label(first neighbour), label(second neighbour))   on a DAG, and
// re-evaluating F for every kOther pixel until nothing changes reaches it -- with all the threads of the workgroup, in as many passes
// as the longest chain of newly absorbed pixels (a thread walks its pixels in sweep order, so chains along a row cost one pass).  The
// region records (absorbed pixels, the last one in PCL's order) are taken once a sweep has converged.
constexpr int kRefTX = 32, kRefTY = 16;   // k_refine_lds: 512 threads, thread (tx, ty) owns a tile of ceil(w/32) x ceil(h/16) <= 32 pixels
constexpr int kRefMaskRegions = 8;         // boxes with at most this many planes take the precomputed-mask form
// does region `a` absorb pixel i when it arrives from writer pixel s (threshold from the writer's depth)?
__device__ __forceinline__ bool refine_fits(const float* models, const float* pts, float dthr, int a, int i, int s) {
  const float* m = models + a * 4;
  const float z = pts[(size_t)s * 3 + 2];
  const float t = dthr * (z * z);
  const float d = fabsf(m[0] * pts[(size_t)i * 3] + m[1] * pts[(size_t)i * 3 + 1] + m[2] * pts[(size_t)i * 3 + 2] + m[3]);
  return d < t;
}
// first / second candidate writer of pixel i in this sweep's order and whether they exist as "current" pixels of the sweep; the first
// writer's own gate (its right neighbour in sweep 1 / its left one in sweep 2, label 0 standing in at column 0, must be a valid pixel)
template <int SWEEP>
__device__ __forceinline__ void refine_writers(const short* Lc, int i, int r, int c, int w, int h, int* s1, int* s2, bool* ok1, bool* ok2) {
  *s1 = SWEEP == 1 ? i - w : i + w;
  *s2 = SWEEP == 1 ? i - 1 : i + 1;
  bool o1 = SWEEP == 1 ? (r >= 1 && c <= w - 2) : (r + 1 <= h - 1);
  if (o1) o1 = SWEEP == 1 ? Lc[*s1 + 1] >= 0 : (c >= 1 ? Lc[*s1 - 1] >= 0 : true);
  *ok1 = o1;
  *ok2 = SWEEP == 1 ? (c >= 1 && r <= h - 2) : (c + 1 <= w - 1 && r >= 1);
}
// label of pixel i given its writers' current labels; MASKED: the distance tests were done once per sweep (bit a of the low / high byte
// of M[i]: region a fits when it arrives from the first / second writer; zero where that writer does not exist)
template <int SWEEP, bool MASKED>
__device__ __forceinline__ int refine_eval(const short* Lc, const unsigned short* M, const float* models, const float* pts, float dthr, int i, int r, int c,
                                           int w, int h, int* writer) {
  *writer = 0;
  if (MASKED) {
    // the mask and both writers' labels in one LDS round trip (clamped addresses; a writer that does not exist has an empty mask byte)
    const int n = w * h;
    const int s1 = SWEEP == 1 ? max(i - w, 0) : min(i + w, n - 1), s2 = SWEEP == 1 ? max(i - 1, 0) : min(i + 1, n - 1);
    const unsigned m = M[i];
    const int a1 = Lc[s1], a2 = Lc[s2];
    if (a1 >= 0 && a1 < kRefMaskRegions && ((m >> a1) & 1u)) { *writer = 1; return a1; }
    if (a2 >= 0 && a2 < kRefMaskRegions && ((m >> (8 + a2)) & 1u)) { *writer = 2; return a2; }
    return kOther;
  }
  int s1, s2; bool ok1, ok2;
  refine_writers<SWEEP>(Lc, i, r, c, w, h, &s1, &s2, &ok1, &ok2);
  if (ok1) {
    const int a1 = Lc[s1];
    if (a1 >= 0 && a1 < kMaxRegions && refine_fits(models, pts, dthr, a1, i, s1)) { *writer = 1; return a1; }
  }
  if (ok2) {
    const int a2 = Lc[s2];
    if (a2 >= 0 && a2 < kMaxRegions && refine_fits(models, pts, dthr, a2, i, s2)) { *writer = 2; return a2; }
  }
  return kOther;
}
template <int SWEEP, bool MASKED>
__device__ __forceinline__ void refine_sweep_lds(short* Lc, unsigned short* M, const float* models, int nregs, const float* pts, float dthr, int w, int h,
                                                 int* s_changed, int* rcnt, unsigned long long* rkey) {
  const int tid = threadIdx.x;
  const int tw = (w + kRefTX - 1) / kRefTX, th = (h + kRefTY - 1) / kRefTY;
  const int c0 = (tid % kRefTX) * tw, r0 = (tid / kRefTX) * th;
  const int c1 = min(w, c0 + tw), r1 = min(h, r0 + th);
  const int tw_inv = 65536 / tw + 1;
  unsigned cand = 0;                            // bit (dy * tw + dx): the pixel carried kOther when the sweep began
  unsigned act = 0;                             // MASKED: ... and some plane fits it from some writer (the others can never change)
  for (int r = r0; r < r1; ++r)
    for (int c = c0; c < c1; ++c) {
      const int i = r * w + c;
      if (Lc[i] < kMaxRegions) continue;
      cand |= 1u << ((r - r0) * tw + (c - c0));
      if (MASKED) {
        int s1, s2; bool ok1, ok2;
        refine_writers<SWEEP>(Lc, i, r, c, w, h, &s1, &s2, &ok1, &ok2);
        unsigned m = 0;
        if (ok1 || ok2) {   // the distance to a plane does not depend on the writer, only the threshold (the writer's depth) does
          const float px = pts[(size_t)i * 3], py = pts[(size_t)i * 3 + 1], pz = pts[(size_t)i * 3 + 2];
          const float z1 = pts[(size_t)(ok1 ? s1 : i) * 3 + 2], z2 = pts[(size_t)(ok2 ? s2 : i) * 3 + 2];
          const float t1 = dthr * (z1 * z1), t2 = dthr * (z2 * z2);
          for (int a = 0; a < nregs; ++a) {
            const float* mm = models + a * 4;
            const float d = fabsf(mm[0] * px + mm[1] * py + mm[2] * pz + mm[3]);
            if (ok1 && d < t1) m |= 1u << a;
            if (ok2 && d < t2) m |= 1u << (8 + a);
          }
        }
        M[i] = (unsigned short)m;
        if (m) act |= 1u << ((r - r0) * tw + (c - c0));
      }
    }
  if (tid < 3) s_changed[tid] = 0;
  __syncthreads();
  for (int pass = 0; pass < w + h + 2; ++pass) {
    // three flags in rotation: pass p raises [p % 3], clears [(p + 1) % 3] (last read before the barrier of pass p - 1): one barrier per pass
    if (tid == 0) s_changed[(pass + 1) % 3] = 0;
    bool ch = false;
    // the tile's live pixels in sweep order (lowest bit first in sweep 1, highest first in sweep 2), so that a chain inside the tile is
    // followed to its end in one pass; k / tw by a reciprocal that is exact for k < 32
    unsigned bits = MASKED ? act : cand;
    while (bits) {
      const int k = SWEEP == 1 ? __ffs((int)bits) - 1 : 31 - __clz((int)bits);
      bits &= ~(1u << k);
      const int dy = (k * tw_inv) >> 16, dx = k - dy * tw;
      const int r = r0 + dy, c = c0 + dx, i = r * w + c;
      int wr;
      const int v = refine_eval<SWEEP, MASKED>(Lc, M, models, pts, dthr, i, r, c, w, h, &wr);
      if (v != Lc[i]) { Lc[i] = (short)v; ch = true; }
    }
    if (ch) s_changed[pass % 3] = 1;
    __syncthreads();
    if (!s_changed[pass % 3]) break;
  }
  __syncthreads();
  for (int r = r0; r < r1; ++r)
    for (int c = c0; c < c1; ++c) {
      const int i = r * w + c;
      if (!((cand >> ((r - r0) * tw + (c - c0))) & 1u) || Lc[i] >= kMaxRegions) continue;
      int wr;
      const int v = refine_eval<SWEEP, MASKED>(Lc, M, models, pts, dthr, i, r, c, w, h, &wr);
      // order key of the writing pixel: its raster position (sweep 1) / reverse raster position (sweep 2), x 2, + 1 for the vertical write
      const int sidx = SWEEP == 1 ? (wr == 1 ? i - w : i - 1) : (wr == 1 ? i + w : i + 1);
      const int sr = sidx / w, sc = sidx - sr * w;
      const unsigned long long pos = SWEEP == 1 ? (unsigned long long)sidx : (unsigned long long)((h - 1 - sr) * w + (w - 1 - sc));
      const unsigned long long key = pos * 2ull + (wr == 1 ? 1ull : 0ull);
      atomicAdd(&rcnt[v], 1);
      atomicMax(&rkey[v], ((unsigned long long)SWEEP << 60) | (key << 24) | (unsigned long long)i);
    }
  __syncthreads();
}
__global__ __launch_bounds__(kRefTX * kRefTY) void k_refine_lds(View V) {
  extern __shared__ short Lc[];                  // labels (-1, 0..63, kOther) as 16-bit words, then the masks
  __shared__ float models[kMaxRegions * 4];
  __shared__ int rcnt[kMaxRegions];
  __shared__ unsigned long long rkey[kMaxRegions];
  __shared__ int s_changed[3];
  constexpr int NT = kRefTX * kRefTY;
  const BoxMeta b = V.box[blockIdx.x];
  const int slot = blockIdx.x;
  const int nregs = V.nreg[slot];
  if (nregs == 0) return;
  const int w = b.w, h = b.h, n = w * h, tid = threadIdx.x;
  unsigned short* M = reinterpret_cast<unsigned short*>(Lc + ((n + 1) & ~1));
  for (int k = tid; k < nregs * 4; k += NT) models[k] = V.reg[(size_t)slot * kMaxRegions + (k >> 2)].model[k & 3];
  if (tid < kMaxRegions) { rcnt[tid] = 0; rkey[tid] = 0; }
  int* L = V.code + b.pix0;
  const float* gp = V.pts + (size_t)b.pix0 * 3;
  for (int i = tid; i < n; i += NT) Lc[i] = (short)L[i];
  __syncthreads();
  if (nregs <= kRefMaskRegions) {
    refine_sweep_lds<1, true>(Lc, M, models, nregs, gp, V.dist_thr, w, h, s_changed, rcnt, rkey);
    refine_sweep_lds<2, true>(Lc, M, models, nregs, gp, V.dist_thr, w, h, s_changed, rcnt, rkey);
  } else {
    refine_sweep_lds<1, false>(Lc, M, models, nregs, gp, V.dist_thr, w, h, s_changed, rcnt, rkey);
    refine_sweep_lds<2, false>(Lc, M, models, nregs, gp, V.dist_thr, w, h, s_changed, rcnt, rkey);
  }
  for (int i = tid; i < n; i += NT) L[i] = Lc[i];
  if (tid < nregs && rcnt[tid] > 0) {
    Region* R = &V.reg[(size_t)slot * kMaxRegions + tid];
    R->inliers += rcnt[tid];
    if (rkey[tid] > R->last_key) R->last_key = rkey[tid];
  }
}

// findLabeledRegionBoundary (Moore trace from the last inlier) + pcl::calculatePolygonArea, one
// thread per region (sequential by nature; float accumulation in contour order).  The code image is
// staged in LDS as bytes when it fits (<= 150k pixels), so the trace does not pay HBM/L2 latency.
template <bool STAGED>
__global__ __launch_bounds__(256) void k_contour(View V) {
  extern __shared__ unsigned char cimg[];   // (w+2) x (h+2) code image with a border of "invalid" (no bounds tests)
  const int bx = blockIdx.x;
  const BoxMeta b = V.box[bx];
  const int w = b.w, h = b.h, W2 = w + 2;
  const int* L = V.code + b.pix0;
  const int nregs = V.nreg[bx];
  if (nregs == 0) return;
  if (STAGED) {
    for (int i = threadIdx.x; i < W2 * (h + 2); i += 256) cimg[i] = 255;
    __syncthreads();
    for (int i = threadIdx.x; i < w * h; i += 256) {
      const int c = L[i];
      const int y = i / w, x = i - y * w;
      cimg[(y + 1) * W2 + x + 1] = c < 0 ? 255 : (c >= kMaxRegions ? 254 : (unsigned char)c);
    }
    __syncthreads();
  }
  const int k = threadIdx.x;
  if (k >= nregs) return;
  Region* R = &V.reg[(size_t)bx * kMaxRegions + k];
  const int start = (int)(R->last_key & 0xffffffull);
  // code of pixel (x, y); out-of-image neighbours read as 255 ("not this label"), which is what PCL's
  // bounds tests amount to in the trace loop; the *seed* test below keeps PCL's explicit bounds test
#define CODE_XY(x, y) (STAGED ? (int)cimg[((y) + 1) * W2 + (x) + 1] \
                              : (((x) < 0 || (x) >= w || (y) < 0 || (y) >= h) ? 255 : (L[(y) * w + (x)] < 0 ? 255 : (L[(y) * w + (x)] >= kMaxRegions ? 254 : L[(y) * w + (x)]))))
  int cx = start % w, cy = start / w, ci = start;
  const int label = CODE_XY(cx, cy);
  int dirn = -1;
#pragma unroll
  for (int d = 0; d < 8; ++d) {
    const int ddx = d == 0 || d == 1 || d == 7 ? -1 : (d == 2 || d == 6 ? 0 : 1);
    const int ddy = d == 1 || d == 2 || d == 3 ? -1 : (d == 0 || d == 4 ? 0 : 1);
    const int x = cx + ddx, y = cy + ddy;
    if (dirn < 0 && x >= 0 && x < w && y >= 0 && y < h && CODE_XY(x, y) != label) dirn = d;
  }
  int count = 0, off = -1;
  if (dirn != -1) {
    // each region owns an equal slice of the box's arena (4*w*h ints); boundaries are far shorter
    const int slice = (4 * w * h) / nregs;
    int* out = V.contour + (size_t)b.pix0 * 4 + (size_t)k * slice;
    off = k * slice;
    out[0] = start;
    count = 1;
    const long guard = 4L * (long)w * h + 8;
    long steps = 0;
    do {
      // 8 independent neighbour reads (no dependent LDS chain), then the first match in scan order dirn+1 .. dirn+8
      unsigned match = 0;
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        const int ddx = d == 0 || d == 1 || d == 7 ? -1 : (d == 2 || d == 6 ? 0 : 1);
        const int ddy = d == 1 || d == 2 || d == 3 ? -1 : (d == 0 || d == 4 ? 0 : 1);
        match |= (CODE_XY(cx + ddx, cy + ddy) == label ? 1u : 0u) << d;
      }
      // rotate so that bit 0 is direction dirn+1; no match at all -> PCL's loop ends on (dirn+8)&7 = dirn
      const unsigned rot = ((match | (match << 8)) >> ((dirn + 1) & 7)) & 0xffu;
      const int nI = rot ? ((dirn + 1 + (__ffs(rot) - 1)) & 7) : dirn;
      const int mdx = nI == 0 || nI == 1 || nI == 7 ? -1 : (nI == 2 || nI == 6 ? 0 : 1);
      const int mdy = nI == 1 || nI == 2 || nI == 3 ? -1 : (nI == 0 || nI == 4 ? 0 : 1);
      dirn = (nI + 4) & 7;
      ci += mdy * w + mdx; cx += mdx; cy += mdy;
      if (count < slice) out[count] = ci;
      ++count;
    } while (ci != start && ++steps < guard);
    if (count > slice) off = -1;   // pathological boundary longer than its slice: area stays 0, region is dropped
  }
  R->contour_n = count;
  R->contour_off = off;
  R->area = 0;
#undef CODE_XY
}

// pcl::calculatePolygonArea over the stored boundary: res += p[i] x p[(i+1) % n] in contour order (float).
// One wave per region: 64 cross products are formed in parallel (coalesced index loads, gathered
// points) and parked in LDS; lanes 0..2 then run the three serial float chains of the chunk.
__global__ __launch_bounds__(64) void k_area(View V) {
  __shared__ float prod[3][64];
  const int bx = blockIdx.x, k = blockIdx.y;
  if (k >= V.nreg[bx]) return;
  const BoxMeta b = V.box[bx];
  Region* R = &V.reg[(size_t)bx * kMaxRegions + k];
  const int n = R->contour_n, off = R->contour_off;
  if (n <= 0 || off < 0) return;
  const int* idx = V.contour + (size_t)b.pix0 * 4 + off;
  const float* pts = V.pts + (size_t)b.pix0 * 3;
  const int lane = threadIdx.x;
  float acc = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    if (i < n) {
      const int a = idx[i], c = idx[(i + 1) % n];
      float c3[3];
      cross3(pts + (size_t)a * 3, pts + (size_t)c * 3, c3);
      prod[0][lane] = c3[0]; prod[1][lane] = c3[1]; prod[2][lane] = c3[2];
    }
    __syncthreads();
    if (lane < 3) {
      const int m = min(64, n - i0);
      for (int q = 0; q < m; ++q) acc += prod[lane][q];
    }
    __syncthreads();
  }
  const float rx = __shfl(acc, 0, 64), ry = __shfl(acc, 1, 64), rz = __shfl(acc, 2, 64);
  if (lane == 0) R->area = sqrtf(rx * rx + ry * ry + rz * rz) * 0.5f;
}


// ---------------------------------------------------------------------------------------------
// RANSAC plane fit: pcl::SACSegmentation(SACMODEL_PLANE, SAC_RANSAC) as used by the
// reference's compute2DConvexHull (plane_segmentation.cpp:639-647).  All `max_iterations + slack`
// hypotheses are scored in parallel — one workgroup per hypothesis, one thread per point with a
// wave-ballot / LDS inlier count — and the sequential adaptive-k logic of pcl::RandomSampleConsensus is
// replayed over the counts afterwards, which selects exactly the hypothesis the sequential loop would.
// Sample triples come from a counter-based hash (see oracle/oracle_seg.c for the deviation note).
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ bool plane_inlier(const float* m, const float* p, float thr) {
  return fabsf(m[0] * p[0] + m[1] * p[1] + m[2] * p[2] + m[3]) < thr;
}
// One hypothesis: the sample triple of (seed, iter) -- the first attempt whose three indices differ and whose points pass PCL's
// collinearity test -- and the unit-normal plane through it.  m: the model (zeros if no attempt gave a sample); returns whether a
// sample was found and its model is finite.
__device__ __forceinline__ bool ransac_draw(const float* P, int n, unsigned long long seed, int iter, float* m) {
  float m0 = 0, m1 = 0, m2 = 0, m3 = 0;
  int good = 0;
  for (int attempt = 0; attempt < 1000 && !good; ++attempt) {
    int id[3];
    for (int j = 0; j < 3; ++j)
      id[j] = (int)(splitmix64(seed ^ ((unsigned long long)iter << 32) ^ ((unsigned long long)attempt << 8) ^ (unsigned long long)j) % (unsigned long long)n);
    if (id[0] == id[1] || id[0] == id[2] || id[1] == id[2]) continue;
    const float* p0 = P + (size_t)id[0] * 3; const float* p1 = P + (size_t)id[1] * 3; const float* p2 = P + (size_t)id[2] * 3;
    const float a0 = p1[0] - p0[0], a1 = p1[1] - p0[1], a2 = p1[2] - p0[2];
    const float b0 = p2[0] - p0[0], b1 = p2[1] - p0[1], b2 = p2[2] - p0[2];
    const float r0 = a0 / b0, r1 = a1 / b1, r2 = a2 / b2;
    if (!((r0 != r1) || (r2 != r1))) continue;
    m0 = a1 * b2 - a2 * b1; m1 = a2 * b0 - a0 * b2; m2 = a0 * b1 - a1 * b0;
    const float nn = sqrtf(m0 * m0 + m1 * m1 + m2 * m2);
    m0 /= nn; m1 /= nn; m2 /= nn;
    m3 = -1 * (m0 * p0[0] + m1 * p0[1] + m2 * p0[2]);
    good = 2;   // a sample was found (whether or not its model is finite)
  }
  m[0] = m0; m[1] = m1; m[2] = m2; m[3] = m3;
  return (good == 2) && isfinite(m0) && isfinite(m3);
}
// pcl::RandomSampleConsensus::computeModel's adaptive loop, one hypothesis at a time, over the state (k, iterations, skipped, best):
// the loop goes on while ransac_loop_open; ransac_loop_take consumes a hypothesis with `count` inliers (< 0: no valid sample) out of
// 1 / one_over_n points and says whether it is the best so far.  Used by the host replay of sslam_seg_ransac_plane and by k_ransac_hyp.
SSLAM_HD bool ransac_loop_open(double k, int iterations, int skipped, int max_iterations) {
  return (double)iterations < k && skipped < max_iterations * 10 && iterations <= max_iterations;
}
SSLAM_HD bool ransac_loop_take(int count, double one_over_n, double log_probability, double& k, int& iterations, int& skipped, int& best) {
  if (count < 0) { ++skipped; return false; }
  const bool better = count > best;
  if (better) {
    best = count;
    const double w = (double)count * one_over_n, eps = 2.220446049250313e-16;
    double p_no = 1.0 - pow(w, 3.0);
    if (p_no < eps) p_no = eps;
    if (p_no > 1.0 - eps) p_no = 1.0 - eps;
    k = log_probability / log(p_no);
  }
  ++iterations;
  return better;
}
__global__ __launch_bounds__(256) void k_ransac_score(const float* __restrict__ pts, int n, float thr, unsigned long long seed,
                                                     float* __restrict__ models, int* __restrict__ counts) {
  __shared__ float m[4];
  __shared__ int ok;
  __shared__ int wsum[4];
  const int iter = blockIdx.x;
  if (threadIdx.x == 0) ok = ransac_draw(pts, n, seed, iter, m);
  __syncthreads();
  int cnt = 0;
  if (ok)
    for (int i = threadIdx.x; i < n; i += 256) cnt += plane_inlier(m, pts + (size_t)i * 3, thr) ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    counts[iter] = ok ? wsum[0] + wsum[1] + wsum[2] + wsum[3] : -1;
    models[iter * 4 + 0] = m[0]; models[iter * 4 + 1] = m[1]; models[iter * 4 + 2] = m[2]; models[iter * 4 + 3] = m[3];
  }
}
// ---- ordered compaction: the i in [0, n) that a predicate keeps, in ascending order (PCL's index order) ------------------------------
// k_count_if (kept per block of 256) -> k_exclusive_scan -> k_write_if (every kept i learns its position from the block's offset and
// wave ballots).  A predicate is a small struct passed by value: keep(i) decides, put(pos, i) emits.  compact_if on the host launches
// the three.
template <class Pred>
__global__ __launch_bounds__(256) void k_count_if(Pred pred, int n, int* __restrict__ block_counts) {
  __shared__ int wsum[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  int c = (i < n && pred.keep(i)) ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
// exclusive scan by one thread (nblocks is small); off may be counts itself
__global__ void k_exclusive_scan(const int* counts, int nblocks, int* off, int* total) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int acc = 0;
  for (int b = 0; b < nblocks; ++b) { const int c = counts[b]; off[b] = acc; acc += c; }
  *total = acc;
}
// the same scan by one workgroup, for compactions over millions of entries (the map cloud's brick and voxel tables): every thread sums
// a run of consecutive blocks, the 1024 sums are scanned in LDS, then every thread writes the offsets of its run.  off may be counts.
__global__ __launch_bounds__(1024) void k_exclusive_scan_wide(const int* counts, int nblocks, int* off, int* total) {
  __shared__ int part[1024];
  const int t = threadIdx.x, run = (nblocks + 1023) / 1024;
  const int b0 = min(t * run, nblocks), b1 = min(b0 + run, nblocks);
  int mine = 0;
  for (int b = b0; b < b1; ++b) mine += counts[b];
  part[t] = mine;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int acc = part[t] - mine;
  for (int b = b0; b < b1; ++b) { const int c = counts[b]; off[b] = acc; acc += c; }
  if (t == 1023) *total = part[1023];
}
template <class Pred>
__global__ __launch_bounds__(256) void k_write_if(Pred pred, int n, const int* __restrict__ block_off) {
  __shared__ int woff[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool in = i < n && pred.keep(i);
  const unsigned long long mask = __ballot(in);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) woff[wave] = __popcll(mask);
  __syncthreads();
  int base = block_off[blockIdx.x];
  for (int w = 0; w < wave; ++w) base += woff[w];
  if (in) pred.put(base + __popcll(mask & ((1ull << lane) - 1ull)), i);
}
struct FlagPred {      // set flags -> their indices
  const unsigned char* flag; int* out; int max_out;
  __device__ bool keep(int i) const { return flag[i]; }
  __device__ void put(int pos, int i) const { if (pos < max_out) out[pos] = i; }
};
struct InlierPred {    // inliers of one plane model -> their indices
  const float* pts; const float* model; float thr; int* out; int max_out;
  __device__ bool keep(int i) const { const float m[4] = {model[0], model[1], model[2], model[3]}; return plane_inlier(m, pts + (size_t)i * 3, thr); }
  __device__ void put(int pos, int i) const { if (pos < max_out) out[pos] = i; }
};
// ---- a15, second half: pcl::ProjectInliers (plane) + 2-D pcl::ConvexHull (plane_segmentation.cpp:648-662) ---------
// projectPoints: mc = (a, b, c, 0) normalised in float, dist = mc . p + d (d is not rescaled, as in PCL), p' = p - mc dist
__global__ __launch_bounds__(256) void k_hull_project(const float* __restrict__ pts, const int* __restrict__ inliers, int n_in,
                                                     float a, float b, float c, float d, float* __restrict__ proj) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_in) return;
  const float nrm = sqrtf(a * a + b * b + c * c);
  const float m0 = a / nrm, m1 = b / nrm, m2 = c / nrm;
  const float* p = pts + (size_t)inliers[k] * 3;
  const float dist = m0 * p[0] + m1 * p[1] + m2 * p[2] + d;
  proj[3 * (size_t)k + 0] = p[0] - m0 * dist;
  proj[3 * (size_t)k + 1] = p[1] - m1 * dist;
  proj[3 * (size_t)k + 2] = p[2] - m2 * dist;
}
// coordinate plane of the hull from the normal of the first / last / middle projected point (PCL performReconstruction2D);
// collinear probes: the middle index walks forward.  meta[0] = 0 xy, 1 yz, 2 xz, -1 degenerate
__global__ void k_hull_axes(const float* __restrict__ proj, int n_in, float thresh, int* __restrict__ meta) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float* p0 = proj; const float* p1 = proj + 3 * (size_t)(n_in - 1);
  double nx = 0, ny = 0, nz = 0, nn = 0;
  for (int m = n_in / 2, tries = 0; tries < n_in; ++tries, m = (m + 1) % n_in) {
    const float* p2 = proj + 3 * (size_t)m;
    const double ax = (double)p1[0] - p0[0], ay = (double)p1[1] - p0[1], az = (double)p1[2] - p0[2];
    const double bx = (double)p2[0] - p0[0], by = (double)p2[1] - p0[1], bz = (double)p2[2] - p0[2];
    nx = ay * bz - az * by; ny = az * bx - ax * bz; nz = ax * by - ay * bx;
    nn = sqrt(nx * nx + ny * ny + nz * nz);
    if (nn > 0) break;
  }
  if (!(nn > 0)) { meta[0] = -1; return; }
  const float tx = fabsf((float)(nx / nn)), ty = fabsf((float)(ny / nn)), tz = fabsf((float)(nz / nn));
  bool xy = true, yz = true, xz = true;
  if (tz > thresh) { xz = false; yz = false; }
  if (tx > thresh) { xz = false; xy = false; }
  if (ty > thresh) { xy = false; yz = false; }
  meta[0] = xy ? 0 : (yz ? 1 : (xz ? 2 : -1));
}
__global__ __launch_bounds__(256) void k_hull_coords(const float* __restrict__ proj, int n_in, const int* __restrict__ meta,
                                                    float* __restrict__ px, float* __restrict__ py) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_in) return;
  const int axes = meta[0];
  px[k] = proj[3 * (size_t)k + (axes == 1 ? 1 : 0)];
  py[k] = proj[3 * (size_t)k + (axes == 0 ? 1 : 2)];
}
// Akl-Toussaint pre-filter: the 8 extreme points (W, SW, S, SE, E, NE, N, NW; ties -> lowest index) span an octagon;
// points strictly inside it (by a margin far above the rounding of the double cross products) cannot be hull vertices.
__device__ __forceinline__ double hull_key(int dir, float x, float y) {
  const double dx = x, dy = y;
  switch (dir) { case 0: return -dx; case 1: return -(dx + dy); case 2: return -dy; case 3: return dx - dy;
                 case 4: return dx; case 5: return dx + dy; case 6: return dy; default: return -(dx - dy); }
}
__global__ __launch_bounds__(256) void k_hull_extreme_partial(const float* __restrict__ px, const float* __restrict__ py, int n_in,
                                                             double* __restrict__ bkey, int* __restrict__ bidx) {
  __shared__ double wk[4][8];
  __shared__ int wi[4][8];
  const int k = blockIdx.x * 256 + threadIdx.x;
  const bool ok = k < n_in;
  const float x = ok ? px[k] : 0.f, y = ok ? py[k] : 0.f;
#pragma unroll
  for (int dir = 0; dir < 8; ++dir) {
    double key = ok ? hull_key(dir, x, y) : -1.0e300;
    int idx = ok ? k : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ok2 = __shfl_down(key, o, 64);
      const int oi = __shfl_down(idx, o, 64);
      if (ok2 > key || (ok2 == key && oi < idx)) { key = ok2; idx = oi; }
    }
    if ((threadIdx.x & 63) == 0) { wk[threadIdx.x >> 6][dir] = key; wi[threadIdx.x >> 6][dir] = idx; }
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int dir = threadIdx.x;
    double key = wk[0][dir]; int idx = wi[0][dir];
    for (int w = 1; w < 4; ++w) if (wk[w][dir] > key || (wk[w][dir] == key && wi[w][dir] < idx)) { key = wk[w][dir]; idx = wi[w][dir]; }
    bkey[(size_t)blockIdx.x * 8 + dir] = key; bidx[(size_t)blockIdx.x * 8 + dir] = idx;
  }
}
// ext[dir] = (x, y) of the extreme point, eidx[dir] its index; ext[16] = margin
__global__ void k_hull_extreme_final(const double* __restrict__ bkey, const int* __restrict__ bidx, int nblk, const float* __restrict__ px,
                                     const float* __restrict__ py, double* __restrict__ ext, int* __restrict__ eidx) {
  const int dir = threadIdx.x;
  if (dir < 8) {
    double key = bkey[dir]; int idx = bidx[dir];
    for (int b = 1; b < nblk; ++b) {
      const double k2 = bkey[(size_t)b * 8 + dir]; const int i2 = bidx[(size_t)b * 8 + dir];
      if (k2 > key || (k2 == key && i2 < idx)) { key = k2; idx = i2; }
    }
    eidx[dir] = idx; ext[2 * dir] = px[idx]; ext[2 * dir + 1] = py[idx];
  }
  __syncthreads();
  if (dir == 0) {
    const double ex = ext[8] - ext[0], ey = ext[13] - ext[5];   // E.x - W.x, N.y - S.y
    ext[16] = 1e-10 * (ex * ex + ey * ey);
  }
}
__device__ __forceinline__ bool hull_keep(const double* __restrict__ ext, float x, float y) {
  const double margin = ext[16];
  int edges = 0;
  bool inside = true;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const double ax = ext[2 * e], ay = ext[2 * e + 1], bx = ext[2 * ((e + 1) & 7)], by = ext[2 * ((e + 1) & 7) + 1];
    if (ax == bx && ay == by) continue;
    ++edges;
    const double cr = (bx - ax) * ((double)y - ay) - (by - ay) * ((double)x - ax);
    if (!(cr > margin)) inside = false;
  }
  return !(inside && edges >= 3);
}
struct HullPred {      // points not strictly inside the octagon -> (x, y, index) candidates
  const float* px; const float* py; const double* ext; float* cx; float* cy; int* ci;
  __device__ bool keep(int i) const { return hull_keep(ext, px[i], py[i]); }
  __device__ void put(int pos, int i) const { cx[pos] = px[i]; cy[pos] = py[i]; ci[pos] = i; }
};
// One workgroup per chunk of <= kHullCap candidates: bitonic sort by (x, y, index) in LDS, Andrew's monotone chain by
// one thread (strict turns, duplicates keep the lowest index).  FINAL: counter-clockwise polygon rotated to start at the
// vertex of smallest angle about the (double mean -> float) vertex centroid, indices only.  Otherwise the chunk's hull
// vertices go back out as candidates of the next round (the hull of a union is the hull of the parts' hulls).
constexpr int kHullCap = 4096;
__device__ __forceinline__ bool hull_less(float ax, float ay, int ai, float bx, float by, int bi) {
  if (ax != bx) return ax < bx;
  if (ay != by) return ay < by;
  return ai < bi;
}
__device__ __forceinline__ int hull_half(float x, float y) { return y < 0 ? 0 : ((y == 0 && x > 0) ? 1 : (y > 0 ? 2 : 3)); }
// (plain functions over the LDS arrays: lambdas capturing __shared__ arrays by reference have miscompiled before)
__device__ __forceinline__ double hull_cross(const float* sx, const float* sy, int o, int a, int b) {
  return ((double)sx[a] - (double)sx[o]) * ((double)sy[b] - (double)sy[o]) - ((double)sy[a] - (double)sy[o]) * ((double)sx[b] - (double)sx[o]);
}
__device__ __forceinline__ bool hull_ang_less(const float* sx, const float* sy, const int* si, float gx, float gy, int p, int q) {
  const float ax = sx[p] - gx, ay = sy[p] - gy, bx = sx[q] - gx, by = sy[q] - gy;
  const int hp = hull_half(ax, ay), hq = hull_half(bx, by);
  if (hp != hq) return hp < hq;
  const double cr = (double)ax * (double)by - (double)ay * (double)bx;
  if (cr != 0) return cr > 0;
  return si[p] < si[q];
}
template <bool FINAL>
__global__ __launch_bounds__(1024) void k_hull_core(const float* __restrict__ cx, const float* __restrict__ cy, const int* __restrict__ ci, int m,
                                                   float* __restrict__ ox, float* __restrict__ oy, int* __restrict__ oi, int* __restrict__ counts) {
  __shared__ float sx[kHullCap], sy[kHullCap];
  __shared__ int si[kHullCap], st[kHullCap];
  const int c0 = blockIdx.x * kHullCap, mc = min(kHullCap, m - c0), tid = threadIdx.x;
  int N = 1;
  while (N < mc) N <<= 1;
  for (int t = tid; t < N; t += 1024) {
    const bool ok = t < mc;
    sx[t] = ok ? cx[c0 + t] : __int_as_float(0x7f800000); sy[t] = ok ? cy[c0 + t] : 0.f; si[t] = ok ? ci[c0 + t] : 0x7fffffff;
  }
  __syncthreads();
  for (int k = 2; k <= N; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < N; t += 1024) {
        const int u = t ^ j;
        if (u > t) {
          const bool asc = (t & k) == 0;
          const bool lt = hull_less(sx[u], sy[u], si[u], sx[t], sy[t], si[t]);   // element u sorts before element t
          if (lt == asc) {
            const float fx = sx[t], fy = sy[t]; const int fi = si[t];
            sx[t] = sx[u]; sy[t] = sy[u]; si[t] = si[u]; sx[u] = fx; sy[u] = fy; si[u] = fi;
          }
        }
      }
      __syncthreads();
    }
  if (tid != 0) return;
  // dedupe in place
  int mu = 0;
  for (int k = 0; k < mc; ++k) {
    if (mu > 0 && sx[k] == sx[mu - 1] && sy[k] == sy[mu - 1]) continue;
    sx[mu] = sx[k]; sy[mu] = sy[k]; si[mu] = si[k]; ++mu;
  }
  int h = 0;
  for (int k = 0; k < mu; ++k) {
    while (h >= 2 && hull_cross(sx, sy, st[h - 2], st[h - 1], k) <= 0) --h;
    st[h++] = k;
  }
  for (int k = mu - 2, t = h + 1; k >= 0; --k) {
    while (h >= t && hull_cross(sx, sy, st[h - 2], st[h - 1], k) <= 0) --h;
    st[h++] = k;
  }
  if (mu > 1) --h;
  if (!FINAL) {
    for (int k = 0; k < h; ++k) { const int p = st[k]; ox[c0 + k] = sx[p]; oy[c0 + k] = sy[p]; oi[c0 + k] = si[p]; }
    counts[blockIdx.x] = h;
    return;
  }
  double sumx = 0, sumy = 0;
  for (int k = 0; k < h; ++k) { sumx += sx[st[k]]; sumy += sy[st[k]]; }
  const float gx = (float)(sumx / h), gy = (float)(sumy / h);
  int first = 0;
  for (int k = 1; k < h; ++k) if (hull_ang_less(sx, sy, si, gx, gy, st[k], st[first])) first = k;
  for (int k = 0; k < h; ++k) oi[k] = si[st[(first + k) % h]];
  counts[0] = h;
}
// compaction between rounds: chunk c's `counts[c]` vertices move to offset off[c]
__global__ __launch_bounds__(256) void k_hull_compact(const float* __restrict__ ox, const float* __restrict__ oy, const int* __restrict__ oi,
                                                     const int* __restrict__ counts, const int* __restrict__ off, float* __restrict__ cx,
                                                     float* __restrict__ cy, int* __restrict__ ci) {
  const int c = blockIdx.x, n = counts[c], o = off[c];
  for (int k = threadIdx.x; k < n; k += 256) { cx[o + k] = ox[c * kHullCap + k]; cy[o + k] = oy[c * kHullCap + k]; ci[o + k] = oi[c * kHullCap + k]; }
}

// optimizeModelCoefficients' last step: the inliers' sums of xx, xy, xz, yy, yz, zz, x, y, z (float, added in index order) -> means,
// covariance, the eigenvector of its smallest eigenvalue as the normal, d = -n . mean
__device__ __forceinline__ void plane_from_moments(const float* sum, int count, float* model) {
  float a[9];
  const float cf = (float)count;
#pragma unroll
  for (int q = 0; q < 9; ++q) a[q] = sum[q] / cf;
  float cov[9];
  cov[0] = a[0] - a[6] * a[6]; cov[1] = a[1] - a[6] * a[7]; cov[2] = a[2] - a[6] * a[8];
  cov[4] = a[3] - a[7] * a[7]; cov[5] = a[4] - a[7] * a[8]; cov[8] = a[5] - a[8] * a[8];
  cov[3] = cov[1]; cov[6] = cov[2]; cov[7] = cov[5];
  float ev, v[3];
  eigen33(cov, ev, v);
  model[0] = v[0]; model[1] = v[1]; model[2] = v[2];
  model[3] = -1 * (v[0] * a[6] + v[1] * a[7] + v[2] * a[8]);
}
// optimizeModelCoefficients: float sums over the inliers in index order + plane_from_moments (one wave)
__global__ __launch_bounds__(64) void k_ransac_refit(const float* __restrict__ pts, const int* __restrict__ inliers, const int* __restrict__ total,
                                                    float* __restrict__ model) {
  __shared__ float prod[64][9];
  const int cntN = *total;
  if (cntN <= 3) return;   // PCL keeps the unrefined model
  const int lane = threadIdx.x;
  float acc = 0;
  for (int i0 = 0; i0 < cntN; i0 += 64) {
    const int i = i0 + lane;
    if (i < cntN) {
      const float* p = pts + (size_t)inliers[i] * 3;
      float* q = prod[lane];
      q[0] = p[0] * p[0]; q[1] = p[0] * p[1]; q[2] = p[0] * p[2]; q[3] = p[1] * p[1]; q[4] = p[1] * p[2]; q[5] = p[2] * p[2];
      q[6] = p[0]; q[7] = p[1]; q[8] = p[2];
    }
    __syncthreads();
    if (lane < 9) { const int mcount = min(64, cntN - i0); for (int q = 0; q < mcount; ++q) acc += prod[q][lane]; }
    __syncthreads();
  }
  float a[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) a[q] = __shfl(acc, q, 64);
  if (lane == 0) plane_from_moments(a, cntN, model);
}

// final label image for the parity hook: region index or -1
__global__ __launch_bounds__(256) void k_label_image(View V, int box, int* out) {
  const BoxMeta b = V.box[box];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= b.w * b.h) return;
  const int c = V.code[b.pix0 + i];
  out[i] = (c >= 0 && c < kMaxRegions) ? c : -1;
}


// ---- point-to-plane ICP (judge row J1; BASELINE.json north_star "RANSAC plane fit + point-to-plane ICP"; no counterpart in the
// reference tree) -------------------------------------------------------------------------------------------------------------------
// One Gauss-Newton round: every labelled point q = R p + t contributes, for its plane (n, d),
//   r = n . q + d,   J = [ (q x n)^T  n^T ]      (update  T <- (exp[w]x, u) o T,  d r / d w = q x n,  d r / d u = n)
// to  J^T J (21 values), J^T r (6), r^2 and the point count (icp_add_point): 29 double sums, reduced per workgroup in a fixed order
// (block_sum4) -> partial[block][29]; the host adds the blocks in order and takes the step (icp_gn_step, csrc/sslam_math.hpp).
struct IcpPose { double T[12]; };   // R row-major, then t
constexpr int kIcpSums = 29;
// the contribution of point p (skipped unless finite) measured against plane (n, d) under the transform (R, t)
__device__ __forceinline__ void icp_add_point(const double* R, const double* t, const float* p, double nx, double ny, double nz, double d,
                                              double (&a)[kIcpSums]) {
  const double px = p[0], py = p[1], pz = p[2];
  if (!(isfinite(px) && isfinite(py) && isfinite(pz))) return;
  const double qx = R[0] * px + R[1] * py + R[2] * pz + t[0];
  const double qy = R[3] * px + R[4] * py + R[5] * pz + t[1];
  const double qz = R[6] * px + R[7] * py + R[8] * pz + t[2];
  const double r = nx * qx + ny * qy + nz * qz + d;
  const double J[6] = {qy * nz - qz * ny, qz * nx - qx * nz, qx * ny - qy * nx, nx, ny, nz};
  int m = 0;
#pragma unroll
  for (int rr = 0; rr < 6; ++rr)
#pragma unroll
    for (int cc = rr; cc < 6; ++cc) a[m++] += J[rr] * J[cc];
#pragma unroll
  for (int rr = 0; rr < 6; ++rr) a[21 + rr] += J[rr] * r;
  a[27] += r * r;
  a[28] += 1.0;
}
// a[K] summed over a 256-thread workgroup in a fixed order -- the shuffle tree of each wave, then the four waves in order -- into out[K]
template <int K>
__device__ __forceinline__ void block_sum4(const double (&a)[K], double (&red)[4][K], double* __restrict__ out) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double v = a[k];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((tid & 63) == 0) red[tid >> 6][k] = v;
  }
  __syncthreads();
  if (tid < K) out[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}
__global__ __launch_bounds__(256) void k_icp_accumulate(const float* __restrict__ xyz, const int* __restrict__ lab, int n,
                                                        const float* __restrict__ planes, int n_planes, IcpPose T, double* __restrict__ partial) {
  __shared__ double red[4][kIcpSums];
  double a[kIcpSums];
#pragma unroll
  for (int k = 0; k < kIcpSums; ++k) a[k] = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int k = lab[i];
    if (k < 0 || k >= n_planes) continue;
    icp_add_point(T.T, T.T + 9, xyz + 3 * (size_t)i, planes[4 * k], planes[4 * k + 1], planes[4 * k + 2], planes[4 * k + 3], a);
  }
  block_sum4(a, red, partial + (size_t)blockIdx.x * kIcpSums);
}


// ---- RANSAC plane per detection box + point-to-plane ICP per frame over the RESIDENT batch (BASELINE.json configs[3]; north_star "RANSAC
// plane fit + point-to-plane ICP over depth clouds inside detection boxes ... one-thread-per-point HIP kernels with LDS inlier counting";
// the only RANSAC hook upstream is compute2DConvexHull, plane_segmentation.cpp:631-665) -------------------------------------------------
// One workgroup per box.  The box's cropped cloud (w x h points in crop order, invalid points included: they are never inliers and a
// sample that hits one is a bad sample) is staged in LDS once -- 12 bytes per point read from HBM once -- and every hypothesis is scored
// out of LDS: sixteen hypotheses at a time, one wave each (lane 0 draws the sample with ransac_draw, as the single-cloud entry
// point does, the wave counts inliers with a point per lane), then one thread runs pcl::RandomSampleConsensus' adaptive loop
// (ransac_loop_open / ransac_loop_take) over the sixteen counts in order and stops the box as soon as the sequential algorithm would
// have stopped.  optimizeModelCoefficients needs float sums over the inliers IN INDEX ORDER: the points are walked 1024 at a time,
// every inlier gets its rank from wave ballots and parks its nine products in LDS, nine lanes add them in rank order -- the arithmetic
// of oracle_seg.c's serial loop, bit for bit.
struct RansacBox { float coeff[4]; int inliers, best_count, best_iter, hyps; };
// Round 6: two kernels.  (PMC, profiles/r6_pmc_frontend.json: the one-kernel form spent 85 % of its wave cycles parked -- nine lanes added
// the inliers' products one LDS round trip at a time while fifteen waves and a 147 KB crop waited, one box per CU.)
//   k_ransac_hyp      one 1024-thread workgroup per box, the crop staged in LDS once.  A round draws up to sixteen samples (one wave each, lane
//                     0, ransac_draw), then ONE pass over the points scores all of them: a thread keeps the
//                     round's models in registers and tests each of its points against every model -- three LDS reads per point instead of
//                     three per point and hypothesis.  Thread 0 replays pcl::RandomSampleConsensus' adaptive loop over the counts in order and
//                     stops where the sequential algorithm stops (rounds after the first draw eight samples: the scene's boxes stop at 17).
//   k_ransac_refine   one 256-thread workgroup per box, eight per CU: optimizeModelCoefficients' float sums over the inliers IN INDEX ORDER
//                     (ranks from wave ballots, nine products parked in LDS, nine lanes add them in rank order, sixteen loads in flight ahead of
//                     the dependent adds) -- the arithmetic of oracle_seg.c's serial loop, bit for bit --, plane_from_moments, then the inlier flags of the
//                     refined model.  The chains of eight boxes overlap on a CU; the points come through L2.
constexpr int kRsProd = 256;   // inlier products parked per round of the ordered sums
constexpr int kRsHyp = 16;     // hypotheses of the first round of a box (later rounds: kRsHyp / 2)
__global__ __launch_bounds__(1024) void k_ransac_hyp(View V, float thr, int max_iterations, double probability, unsigned long long seed0,
                                                     int lds_points, RansacBox* __restrict__ out) {
  extern __shared__ float sp[];
  __shared__ float s_models[kRsHyp][4];
  __shared__ int s_cnt[kRsHyp], s_ok[kRsHyp];
  __shared__ float s_best[4];
  __shared__ int s_stop, s_best_n, s_best_it, s_it;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const BoxMeta b = V.box[blockIdx.x];
  const int n = b.w * b.h;
  const float* gp = V.pts + (size_t)b.pix0 * 3;
  const bool staged = n <= lds_points;
  if (staged) {
    if ((((size_t)b.pix0 * 3) & 3) == 0) {   // 16-byte pieces where the crop starts on one
      const float4* g4 = reinterpret_cast<const float4*>(gp);
      float4* s4 = reinterpret_cast<float4*>(sp);
      const int n4 = (3 * n) >> 2;
      for (int e = tid; e < n4; e += 1024) s4[e] = g4[e];
      for (int e = 4 * n4 + tid; e < 3 * n; e += 1024) sp[e] = gp[e];
    } else {
      for (int e = tid; e < 3 * n; e += 1024) sp[e] = gp[e];
    }
  }
  const float* P = staged ? (const float*)sp : gp;
  const unsigned long long seed = seed0 + (unsigned long long)blockIdx.x * 0x9E3779B97F4A7C15ull;
  if (tid == 0) { s_stop = n < 3 ? 1 : 0; s_best_n = -1; s_best_it = -1; s_it = 0; s_best[0] = s_best[1] = s_best[2] = s_best[3] = 0; }
  __syncthreads();
  // the adaptive loop's state lives in thread 0
  double k = 1.0;
  int iterations = 0, skipped = 0;
  const double log_probability = log(1.0 - probability), one_over = 1.0 / (double)n;
  int nh = kRsHyp;
  while (!s_stop) {
    if (wave < nh && lane == 0) {
      s_ok[wave] = ransac_draw(P, n, seed, s_it + wave, s_models[wave]);
      s_cnt[wave] = 0;
    }
    __syncthreads();
    {   // one pass over the points for all hypotheses of the round
      float m[kRsHyp][4];
      int cnt[kRsHyp];
#pragma unroll
      for (int h = 0; h < kRsHyp; ++h) {
        const int hh = h < nh ? h : 0;
        m[h][0] = s_models[hh][0]; m[h][1] = s_models[hh][1]; m[h][2] = s_models[hh][2]; m[h][3] = s_models[hh][3];
        cnt[h] = 0;
      }
      if (nh == kRsHyp) {
        for (int i = tid; i < n; i += 1024) {
          const float p[3] = {P[(size_t)i * 3], P[(size_t)i * 3 + 1], P[(size_t)i * 3 + 2]};
#pragma unroll
          for (int h = 0; h < kRsHyp; ++h) cnt[h] += plane_inlier(m[h], p, thr) ? 1 : 0;
        }
      } else {
        for (int i = tid; i < n; i += 1024) {
          const float p[3] = {P[(size_t)i * 3], P[(size_t)i * 3 + 1], P[(size_t)i * 3 + 2]};
#pragma unroll
          for (int h = 0; h < kRsHyp / 2; ++h) cnt[h] += plane_inlier(m[h], p, thr) ? 1 : 0;
        }
      }
#pragma unroll
      for (int h = 0; h < kRsHyp; ++h) {
        if (h < nh) {
          int c = cnt[h];
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
          if (lane == 0) atomicAdd(&s_cnt[h], c);     // integer counts: the order of the waves does not matter
        }
      }
    }
    __syncthreads();
    if (tid == 0) {   // pcl::RandomSampleConsensus::computeModel over these hypotheses, in order
      int stop = 0;
      for (int j = 0; j < nh; ++j) {
        if (!ransac_loop_open(k, iterations, skipped, max_iterations)) { stop = 1; break; }
        if (ransac_loop_take(s_ok[j] ? s_cnt[j] : -1, one_over, log_probability, k, iterations, skipped, s_best_n)) {
          s_best_it = s_it;
          s_best[0] = s_models[j][0]; s_best[1] = s_models[j][1]; s_best[2] = s_models[j][2]; s_best[3] = s_models[j][3];
        }
        ++s_it;
      }
      s_stop = stop || iterations > max_iterations;
    }
    nh = kRsHyp / 2;
    __syncthreads();
  }
  if (tid == 0) out[blockIdx.x] = RansacBox{{s_best[0], s_best[1], s_best[2], s_best[3]}, 0, s_best_n, s_best_it, s_it};
}

__global__ __launch_bounds__(256) void k_ransac_refine(View V, float thr, RansacBox* __restrict__ out, unsigned char* __restrict__ flag) {
  __shared__ float prod[kRsProd * 9];
  __shared__ int s_woff[5];
  __shared__ float s_best[4], s_acc[9];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const BoxMeta b = V.box[blockIdx.x];
  const int n = b.w * b.h;
  const float* P = V.pts + (size_t)b.pix0 * 3;
  const RansacBox rb = out[blockIdx.x];
  const int best = rb.best_count;
  float model[4] = {rb.coeff[0], rb.coeff[1], rb.coeff[2], rb.coeff[3]};
  if (best <= 0) {
    for (int i = tid; i < n; i += 256) flag[(size_t)b.pix0 + i] = 0;
    if (tid == 0) out[blockIdx.x] = RansacBox{{0, 0, 0, 0}, 0, best, rb.best_iter, rb.hyps};
    return;
  }
  // ---- optimizeModelCoefficients: float mean / covariance of the inliers of the sampled model, summed in index order
  if (best > 3) {
    float acc = 0;
    int total = 0;
    for (int c0 = 0; c0 < n; c0 += kRsProd) {
      const int i = c0 + tid;
      float p[3] = {0, 0, 0};
      if (i < n) { p[0] = P[(size_t)i * 3]; p[1] = P[(size_t)i * 3 + 1]; p[2] = P[(size_t)i * 3 + 2]; }
      const bool in = i < n && plane_inlier(model, p, thr);
      const unsigned long long mask = __ballot(in);
      if (lane == 0) s_woff[wave] = __popcll(mask);
      __syncthreads();
      const int w0 = s_woff[0], w1 = s_woff[1], w2 = s_woff[2], w3 = s_woff[3];
      const int cn = w0 + w1 + w2 + w3;
      const int rank = (wave > 0 ? w0 : 0) + (wave > 1 ? w1 : 0) + (wave > 2 ? w2 : 0) + __popcll(mask & ((1ull << lane) - 1ull));
      if (in) {
        float* q = prod + rank * 9;
        q[0] = p[0] * p[0]; q[1] = p[0] * p[1]; q[2] = p[0] * p[2]; q[3] = p[1] * p[1]; q[4] = p[1] * p[2]; q[5] = p[2] * p[2];
        q[6] = p[0]; q[7] = p[1]; q[8] = p[2];
      }
      __syncthreads();
      if (tid < 9) {   // sixteen loads ahead of sixteen dependent adds: the chain is the adds, not LDS round trips
        int q = 0;
        for (; q + 16 <= cn; q += 16) {
          float v[16];
#pragma unroll
          for (int u = 0; u < 16; ++u) v[u] = prod[(q + u) * 9 + tid];
#pragma unroll
          for (int u = 0; u < 16; ++u) acc += v[u];
        }
        for (; q < cn; ++q) acc += prod[q * 9 + tid];
      }
      __syncthreads();
      total += cn;
    }
    if (tid < 9) s_acc[tid] = acc;
    __syncthreads();
    if (tid == 0) plane_from_moments(s_acc, total, s_best);
    __syncthreads();
    model[0] = s_best[0]; model[1] = s_best[1]; model[2] = s_best[2]; model[3] = s_best[3];
  }
  // ---- inliers of the refined model: flags for the box's pixels + their count
  int cnt = 0;
  for (int i = tid; i < n; i += 256) {
    const bool in = plane_inlier(model, P + (size_t)i * 3, thr);
    flag[(size_t)b.pix0 + i] = in ? 1 : 0;
    cnt += in ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
  __syncthreads();
  if (lane == 0) s_woff[wave] = cnt;
  __syncthreads();
  if (tid == 0) out[blockIdx.x] = RansacBox{{model[0], model[1], model[2], model[3]}, s_woff[0] + s_woff[1] + s_woff[2] + s_woff[3], best, rb.best_iter, rb.hyps};
}

// Point-to-plane ICP of every frame of the resident batch against a plane list (e.g. the previous keyframe's planes): the points are the
// RANSAC inliers of the frame's boxes, box slot q measures plane box_plane[q] (-1: the box takes no part).
// Round 4 ran ONE 1024-thread workgroup per frame through all Gauss-Newton rounds: 32 workgroups on 256 CUs, 0.234 ms per frame -- 2.7 x
// the whole segmentation.  Round 5: a Gauss-Newton round is two launches over the whole batch --
//   k_icp_box_sums    one workgroup per BOX: its inliers' 29 double sums under the frame's current transform (fixed-order reduction:
//                     a thread's points in index order, wave shuffles, the waves in order) -> part[box][29]
//   k_icp_frame_step  one wave per FRAME: the boxes' partial sums in slot order, the 6 x 6 Cholesky solve and T <- (exp[w]x, u) o T by
//                     lane 0; a frame that is finished (last pass, < 6 points, rank-deficient plane set) is frozen by its flag
// -- 2 (iterations + 1) launches of a few microseconds for ALL frames, still no host round trip per iteration.  The point's row is
// icp_add_point and the step is icp_gn_step (csrc/sslam_math.hpp), the ones of k_icp_accumulate and sslam_seg_icp_point_to_plane; only
// the order of the sums differs.
struct IcpFrame { double T[12]; double rms; int used, status; };
struct IcpState { double T[12]; int status, done, pad0, pad1; };
__global__ __launch_bounds__(256) void k_icp_box_sums(View V, const unsigned char* __restrict__ flag, const int* __restrict__ box_frame,
                                                      const int* __restrict__ box_plane, const float* __restrict__ planes, int n_planes,
                                                      const IcpState* __restrict__ st, double* __restrict__ part) {
  __shared__ double red[4][kIcpSums];
  const int q = blockIdx.x, tid = threadIdx.x;
  const int f = box_frame[q], kpl = box_plane[q];
  double a[kIcpSums];
#pragma unroll
  for (int k = 0; k < kIcpSums; ++k) a[k] = 0.0;
  if (!st[f].done && kpl >= 0 && kpl < n_planes) {
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = st[f].T[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = st[f].T[9 + k];
    const BoxMeta b = V.box[q];
    const double nx = planes[4 * kpl], ny = planes[4 * kpl + 1], nz = planes[4 * kpl + 2], d = planes[4 * kpl + 3];
    const int n = b.w * b.h;
    for (int i = tid; i < n; i += 256) {
      if (!flag[(size_t)b.pix0 + i]) continue;
      icp_add_point(R, t, V.pts + ((size_t)b.pix0 + i) * 3, nx, ny, nz, d, a);
    }
  }
  block_sum4(a, red, part + (size_t)q * kIcpSums);
}
__global__ __launch_bounds__(64) void k_icp_frame_step(const int* __restrict__ frame_box0, const double* __restrict__ part, int it, int iterations,
                                                       IcpState* __restrict__ st, IcpFrame* __restrict__ out) {
  __shared__ double sums[kIcpSums];
  const int f = blockIdx.x, tid = threadIdx.x;
  if (st[f].done) return;
  if (tid < kIcpSums) {
    double v = 0;
    for (int q = frame_box0[f]; q < frame_box0[f + 1]; ++q) v += part[(size_t)q * kIcpSums + tid];   // slot order
    sums[tid] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  IcpState S = st[f];
  if (it == iterations || sums[28] < 6 || S.status) {   // the last pass only measures the residual at the returned transform
    IcpFrame o;
    for (int k = 0; k < 12; ++k) o.T[k] = S.T[k];
    o.rms = sums[28] > 0 ? sqrt(sums[27] / sums[28]) : 0.0;
    o.used = (int)sums[28]; o.status = S.status;
    out[f] = o;
    st[f].done = 1;
    return;
  }
  if (!icp_gn_step(sums, S.T)) { st[f].status = SSLAM_ERR_NUMERIC; return; }   // the planes leave a degree of freedom unconstrained: the next pass reports it
  for (int k = 0; k < 12; ++k) st[f].T[k] = S.T[k];
}

// ---- cloud filters of the legacy path (plane_segmentation.cpp:557-629) ---------------------------------------------
// (their index lists come from the ordered compaction above with FlagPred)
// distance_filter (plane_segmentation.cpp:607-629): keep p with 0.3 < |p| < 3 (float norm, compared as double)
__global__ __launch_bounds__(256) void k_range_flag(const float* __restrict__ pts, int n, double dmin, double dmax, unsigned char* __restrict__ flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
  const double d = (double)sqrtf((x * x + y * y) + z * z);
  flag[i] = (d > dmin && d < dmax) ? 1 : 0;
}
// pcl::VoxelGrid (leaf 0.1, plane_segmentation.cpp:565-581).  Bounding box of the finite points: per-block float min / max
__global__ __launch_bounds__(256) void k_voxel_minmax(const float* __restrict__ pts, int n, float* __restrict__ part) {
  __shared__ float red[4][6];
  float lo[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f}, hi[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) continue;
    lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
    hi[0] = fmaxf(hi[0], x); hi[1] = fmaxf(hi[1], y); hi[2] = fmaxf(hi[2], z);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
    for (int o = 32; o > 0; o >>= 1) { lo[k] = fminf(lo[k], __shfl_down(lo[k], o, 64)); hi[k] = fmaxf(hi[k], __shfl_down(hi[k], o, 64)); }
  if ((threadIdx.x & 63) == 0) for (int k = 0; k < 3; ++k) { red[threadIdx.x >> 6][k] = lo[k]; red[threadIdx.x >> 6][3 + k] = hi[k]; }
  __syncthreads();
  if (threadIdx.x < 3) part[blockIdx.x * 6 + threadIdx.x] = fminf(fminf(red[0][threadIdx.x], red[1][threadIdx.x]), fminf(red[2][threadIdx.x], red[3][threadIdx.x]));
  else if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = fmaxf(fmaxf(red[0][threadIdx.x], red[1][threadIdx.x]), fmaxf(red[2][threadIdx.x], red[3][threadIdx.x]));
}
struct VoxelGeom { float inv[3]; int minb[3]; int mul[3]; };
// cell of every finite point; per cell: point count and the coordinate sums in 2^-20 fixed point (integer atomics: exact and
// independent of the order in which the points arrive -- PCL's own accumulation order is that of an unstable sort)
__global__ __launch_bounds__(256) void k_voxel_accumulate(const float* __restrict__ pts, int n, VoxelGeom G, int* __restrict__ count, long long* __restrict__ sums) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return;
  const int ix = (int)floorf(x * G.inv[0]) - G.minb[0], iy = (int)floorf(y * G.inv[1]) - G.minb[1], iz = (int)floorf(z * G.inv[2]) - G.minb[2];
  const size_t c = (size_t)ix * G.mul[0] + (size_t)iy * G.mul[1] + (size_t)iz * G.mul[2];
  atomicAdd(&count[c], 1);
  atomicAdd((unsigned long long*)&sums[3 * c], (unsigned long long)llrint((double)x * 1048576.0));
  atomicAdd((unsigned long long*)&sums[3 * c + 1], (unsigned long long)llrint((double)y * 1048576.0));
  atomicAdd((unsigned long long*)&sums[3 * c + 2], (unsigned long long)llrint((double)z * 1048576.0));
}
__global__ __launch_bounds__(256) void k_voxel_flag(const int* __restrict__ count, int ncell, unsigned char* __restrict__ flag) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < ncell) flag[c] = count[c] > 0;
}
__global__ __launch_bounds__(256) void k_voxel_centroids(const int* __restrict__ cells, int nocc, const int* __restrict__ count, const long long* __restrict__ sums,
                                                        float* __restrict__ out, int* __restrict__ out_count) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= nocc) return;
  const int c = cells[k], m = count[c];
#pragma unroll
  for (int d = 0; d < 3; ++d) out[3 * (size_t)k + d] = (float)(((double)sums[3 * (size_t)c + d] / 1048576.0) / (double)m);
  if (out_count) out_count[k] = m;
}
// ---- map cloud: many clouds, each at its pose, into one sparse voxel grid (hdl_graph_slam's MapCloudGenerator::generate [UPSTREAM]) ------
// Launch geometry of the three point passes: blockIdx.x = the cloud, blockIdx.y strides over its points in blocks of 256, so a workgroup
// never spans two clouds and R, t are uniform in the wave.  Every pass recomputes the transform (12 B read per point) with the
// arithmetic of k_nn_pairs; a point takes part when its three coordinates and its three transformed coordinates are finite.
struct MapIn { const float* xyz; const int* start; const float* pose; };   // pose: 12 floats per cloud, R row-major then t
__device__ __forceinline__ bool map_point(const MapIn& M, const float* R, int p, float& tx, float& ty, float& tz) {
  const float* q = M.xyz + 3 * (size_t)p;
  const float x = q[0], y = q[1], z = q[2];
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
  tx = ((R[0] * x + R[1] * y) + R[2] * z) + R[9];
  ty = ((R[3] * x + R[4] * y) + R[5] * z) + R[10];
  tz = ((R[6] * x + R[7] * y) + R[8] * z) + R[11];
  return isfinite(tx) && isfinite(ty) && isfinite(tz);
}
// a float as an int of the same order (-0 sorts below +0; both floor to cell 0)
__device__ __forceinline__ int map_ordered(float f) { const int i = __float_as_int(f); return i ^ ((i >> 31) & 0x7fffffff); }
// bounding box of the transformed points: box[0..2] = min, box[3..5] = max, as ordered ints (integer atomics, one set per workgroup; the
// host keeps the launch at about 2048 workgroups: every one of them ends on the same six addresses)
__global__ __launch_bounds__(256) void k_map_minmax(MapIn M, int* __restrict__ box) {
  __shared__ float red[4][6];
  const int c = blockIdx.x, p0 = M.start[c], n = M.start[c + 1] - p0;
  float R[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) R[k] = M.pose[12 * (size_t)c + k];
  float lo[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f}, hi[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
  bool any = false;
  for (int i = blockIdx.y * 256 + threadIdx.x; i < n; i += gridDim.y * 256) {
    float t[3];
    if (!map_point(M, R, p0 + i, t[0], t[1], t[2])) continue;
    any = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], t[k]); hi[k] = fmaxf(hi[k], t[k]); }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
    for (int o = 32; o > 0; o >>= 1) { lo[k] = fminf(lo[k], __shfl_down(lo[k], o, 64)); hi[k] = fmaxf(hi[k], __shfl_down(hi[k], o, 64)); }
  if ((threadIdx.x & 63) == 0) for (int k = 0; k < 3; ++k) { red[threadIdx.x >> 6][k] = lo[k]; red[threadIdx.x >> 6][3 + k] = hi[k]; }
  if (__syncthreads_or(any) == 0) return;   // no usable point in this workgroup
  const int k = threadIdx.x;
  if (k < 3) atomicMin(&box[k], map_ordered(fminf(fminf(red[0][k], red[1][k]), fminf(red[2][k], red[3][k]))));
  else if (k < 6) atomicMax(&box[k], map_ordered(fmaxf(fmaxf(red[0][k], red[1][k]), fmaxf(red[2][k], red[3][k]))));
}
// G: inv, and minb / mul of the dense grid of BRICKS (8 x 8 x 8 cells).  Cell i = (int)floorf(x' * inv) is global; brick i >> 3, local i & 7.
__device__ __forceinline__ void map_cell(const VoxelGeom& G, float tx, float ty, float tz, size_t& brick, int& local) {
  const int ix = (int)floorf(tx * G.inv[0]), iy = (int)floorf(ty * G.inv[1]), iz = (int)floorf(tz * G.inv[2]);
  brick = (size_t)((ix >> 3) - G.minb[0]) * G.mul[0] + (size_t)((iy >> 3) - G.minb[1]) * G.mul[1] + (size_t)((iz >> 3) - G.minb[2]) * G.mul[2];
  local = (ix & 7) | ((iy & 7) << 3) | ((iz & 7) << 6);
}
// pass 1: the occupied bricks
__global__ __launch_bounds__(256) void k_map_flag_bricks(MapIn M, VoxelGeom G, unsigned char* __restrict__ flag) {
  const int c = blockIdx.x, p0 = M.start[c], n = M.start[c + 1] - p0;
  float R[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) R[k] = M.pose[12 * (size_t)c + k];
  for (int i = blockIdx.y * 256 + threadIdx.x; i < n; i += gridDim.y * 256) {
    float tx, ty, tz;
    if (!map_point(M, R, p0 + i, tx, ty, tz)) continue;
    size_t b; int l;
    map_cell(G, tx, ty, tz, b, l);
    flag[b] = 1;
  }
}
struct BrickPred {     // occupied bricks -> their ascending list and the brick -> slot table
  const unsigned char* flag; int* list; int* slot;
  __device__ bool keep(int i) const { return flag[i]; }
  __device__ void put(int pos, int i) const { list[pos] = i; slot[i] = pos; }
};
// pass 2: per voxel slot * 512 + local the point count and the sums of x', y', z' in 2^-20 fixed point, as k_voxel_accumulate keeps them
// (direct form: one 32-bit and three 64-bit integer atomics per point.  Merging runs of equal voxels inside a wave before the atomic
// measured no faster, DESIGN.md section 4: a downsampled cloud has about one point per voxel, the sharing is between clouds, and those
// sit in different workgroups); used: the points that landed, one add per wave
__global__ __launch_bounds__(256) void k_map_accumulate(MapIn M, VoxelGeom G, const int* __restrict__ slot, int* __restrict__ count,
                                                       long long* __restrict__ sums, int* __restrict__ used) {
  const int c = blockIdx.x, p0 = M.start[c], n = M.start[c + 1] - p0;
  float R[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) R[k] = M.pose[12 * (size_t)c + k];
  int mine = 0;
  for (int i = blockIdx.y * 256 + threadIdx.x; i < n; i += gridDim.y * 256) {
    float tx, ty, tz;
    if (!map_point(M, R, p0 + i, tx, ty, tz)) continue;
    size_t b; int l;
    map_cell(G, tx, ty, tz, b, l);
    const size_t v = (size_t)slot[b] * 512 + l;
    atomicAdd(&count[v], 1);
    atomicAdd((unsigned long long*)&sums[3 * v], (unsigned long long)llrint((double)tx * 1048576.0));
    atomicAdd((unsigned long long*)&sums[3 * v + 1], (unsigned long long)llrint((double)ty * 1048576.0));
    atomicAdd((unsigned long long*)&sums[3 * v + 2], (unsigned long long)llrint((double)tz * 1048576.0));
    ++mine;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(used, mine);
}
struct VoxelPred {     // voxels with at least `thr` points -> their ascending list (out may be NULL: count only)
  const int* count; int thr; int* out; int max_out;
  __device__ bool keep(int i) const { return count[i] >= thr; }
  __device__ void put(int pos, int i) const { if (pos < max_out) out[pos] = i; }
};
// pass 3: one record per kept voxel: centroid, global cell, count
__global__ __launch_bounds__(256) void k_map_emit(const int* __restrict__ voxels, int m, const int* __restrict__ bricks, VoxelGeom G, int divx, int divy,
                                                 const int* __restrict__ count, const long long* __restrict__ sums, float* __restrict__ out,
                                                 int* __restrict__ out_cell, int* __restrict__ out_count) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= m) return;
  const int v = voxels[k], n = count[v], l = v & 511, b = bricks[v >> 9];
  const int bx = b % divx + G.minb[0], by = (b / divx) % divy + G.minb[1], bz = b / divx / divy + G.minb[2];
#pragma unroll
  for (int d = 0; d < 3; ++d) out[3 * (size_t)k + d] = (float)(((double)sums[3 * (size_t)v + d] / 1048576.0) / (double)n);
  out_cell[3 * (size_t)k] = bx * 8 + (l & 7); out_cell[3 * (size_t)k + 1] = by * 8 + ((l >> 3) & 7); out_cell[3 * (size_t)k + 2] = bz * 8 + (l >> 6);
  out_count[k] = n;
}
// ---- occupancy map: every point of the map cloud's input is the end of a ray from its cloud's sensor origin (sslam_seg_occupancy_map in
// include/sslam.h states the traversal; octomap_server in the reference's launch [UPSTREAM]) ---------------------------------------------
// Launch geometry, MapIn and map_point are the map cloud's.  The ray origin is uniform in the workgroup; each pass sets its rays up again.
struct OccDev { float inv, z_min, z_max; float org[3]; int R; };      // R: max_range in 1/1024 cell, 1 .. 2^20
struct OccRay { int c[3], e[3], q[3], D[3]; bool cut; };              // start cell, end cell, sub-cell position of the origin, Qe - Qo (|D_a| <= R)
__device__ __forceinline__ bool occ_far(float u) { return !(fabsf(u) < 524288.0f); }
__device__ __forceinline__ long long occ_position(float u) {
  const float fl = floorf(u);
  return (long long)(int)fl * 1024 + min((int)((u - fl) * 1024.0f), 1023);
}
// the ray origin of cloud c: false when it is not finite (the cloud takes no part); far: it lies beyond 2^19 cells
__device__ __forceinline__ bool occ_origin(const float* R, const OccDev& P, long long Qo[3], bool& far) {
  const float x = P.org[0], y = P.org[1], z = P.org[2];
  const float o[3] = {((R[0] * x + R[1] * y) + R[2] * z) + R[9], ((R[3] * x + R[4] * y) + R[5] * z) + R[10], ((R[6] * x + R[7] * y) + R[8] * z) + R[11]};
  far = false;
  if (!(isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]))) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float u = o[k] * P.inv;
    far |= occ_far(u);
    Qo[k] = far ? 0 : occ_position(u);
  }
  return true;
}
enum { OCC_RAY = 0, OCC_NOT_FINITE = 1, OCC_CLIPPED_Z = 2, OCC_FAR = 3 };
__device__ __forceinline__ int occ_ray(const MapIn& M, const float* R, const OccDev& P, const long long Qo[3], bool org_far, int p, OccRay& r) {
  float t[3];
  if (!map_point(M, R, p, t[0], t[1], t[2])) return OCC_NOT_FINITE;
  if (!(t[2] >= P.z_min && t[2] <= P.z_max)) return OCC_CLIPPED_Z;
  if (org_far) return OCC_FAR;
  long long D[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float u = t[k] * P.inv;
    if (occ_far(u)) return OCC_FAR;
    D[k] = occ_position(u) - Qo[k];                       // |Q| <= 2^29, |D| <= 2^30, |D|^2 < 2^62
  }
  const long long len2 = D[0] * D[0] + D[1] * D[1] + D[2] * D[2];
  r.cut = len2 > (long long)P.R * P.R;
  if (r.cut) {
    long long L = (long long)ceil(sqrt((double)len2));
    while (L * L < len2) ++L;
    while ((L - 1) * (L - 1) >= len2) --L;
#pragma unroll
    for (int k = 0; k < 3; ++k) D[k] = (D[k] * P.R) / L;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const long long Qe = Qo[k] + D[k];
    r.c[k] = (int)(Qo[k] >> 10); r.e[k] = (int)(Qe >> 10); r.q[k] = (int)(Qo[k] & 1023); r.D[k] = (int)D[k];
  }
  return OCC_RAY;
}
// the walk: visit(cx, cy, cz, last) for the start cell and every cell stepped into.  num and |D| fit 32 bits (num <= 1024 * 1026,
// |D| <= 2^20), their cross products 64.  The lanes of a wave walk rays of different lengths: the loop runs to the longest, the
// finished lanes masked off.  Returns the cells visited.
template <class Visit>
__device__ __forceinline__ int occ_walk(const OccRay& r, Visit&& visit) {
  int cx = r.c[0], cy = r.c[1], cz = r.c[2];
  int lx = abs(r.e[0] - cx), ly = abs(r.e[1] - cy), lz = abs(r.e[2] - cz);
  const int sx = r.D[0] > 0 ? 1 : -1, sy = r.D[1] > 0 ? 1 : -1, sz = r.D[2] > 0 ? 1 : -1;
  const int dx = abs(r.D[0]), dy = abs(r.D[1]), dz = abs(r.D[2]);
  int nx = r.D[0] > 0 ? 1024 - r.q[0] : r.q[0], ny = r.D[1] > 0 ? 1024 - r.q[1] : r.q[1], nz = r.D[2] > 0 ? 1024 - r.q[2] : r.q[2];
  const int total = lx + ly + lz;
  for (int s = 0; s < total; ++s) {
    visit(cx, cy, cz, false);
    const bool xo = lx > 0, yo = ly > 0, zo = lz > 0;
    const bool xy = xo && (!yo || (long long)nx * dy <= (long long)ny * dx);          // x before y: a tie goes to the lower axis
    const bool xz = !zo || (long long)nx * dz <= (long long)nz * dx;
    const bool yz = !zo || (long long)ny * dz <= (long long)nz * dy;
    if (xy && xz) { cx += sx; nx += 1024; --lx; }
    else if (!xy && yo && yz) { cy += sy; ny += 1024; --ly; }
    else { cz += sz; nz += 1024; --lz; }
  }
  visit(cx, cy, cz, true);
  return total + 1;
}
// pass 0.  box[0..2] / box[3..5]: min / max over the start and end cells of the rays that take part; box[6..9]: those rays, the truncated
// among them, the rows outside the z range, the rows beyond 2^19 cells.  Reduced in the wave and the workgroup, then integer atomics.
__global__ __launch_bounds__(256) void k_occ_minmax(MapIn M, OccDev P, int* __restrict__ box) {
  __shared__ int red[4][10];
  const int c = blockIdx.x, p0 = M.start[c], n = M.start[c + 1] - p0;
  float R[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) R[k] = M.pose[12 * (size_t)c + k];
  long long Qo[3]; bool org_far;
  if (!occ_origin(R, P, Qo, org_far)) return;
  int v[10] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN, 0, 0, 0, 0};
  for (int i = blockIdx.y * 256 + threadIdx.x; i < n; i += gridDim.y * 256) {
    OccRay r;
    const int what = occ_ray(M, R, P, Qo, org_far, p0 + i, r);
    if (what == OCC_CLIPPED_Z) ++v[8];
    if (what == OCC_FAR) ++v[9];
    if (what != OCC_RAY) continue;
    ++v[6];
    if (r.cut) ++v[7];
#pragma unroll
    for (int k = 0; k < 3; ++k) { v[k] = min(v[k], min(r.c[k], r.e[k])); v[3 + k] = max(v[3 + k], max(r.c[k], r.e[k])); }
  }
#pragma unroll
  for (int k = 0; k < 10; ++k)
    for (int o = 32; o > 0; o >>= 1) {
      const int w = __shfl_down(v[k], o, 64);
      v[k] = k < 3 ? min(v[k], w) : k < 6 ? max(v[k], w) : v[k] + w;
    }
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 10; ++k) red[threadIdx.x >> 6][k] = v[k];
  __syncthreads();
  const int k = threadIdx.x;
  if (k >= 10) return;
  const int a = red[0][k], b = red[1][k], d = red[2][k], e = red[3][k];
  if (k < 3) atomicMin(&box[k], min(min(a, b), min(d, e)));
  else if (k < 6) atomicMax(&box[k], max(max(a, b), max(d, e)));
  else if (a + b + d + e) atomicAdd(&box[k], a + b + d + e);
}
// G: minb / mul of the dense grid of BRICKS, as for map_cell
__device__ __forceinline__ size_t occ_brick(const VoxelGeom& G, int cx, int cy, int cz) {
  return (size_t)((cx >> 3) - G.minb[0]) * G.mul[0] + (size_t)((cy >> 3) - G.minb[1]) * G.mul[1] + (size_t)((cz >> 3) - G.minb[2]) * G.mul[2];
}
// pass 1: every brick a ray enters; a byte is stored only when the brick changes
__global__ __launch_bounds__(256) void k_occ_flag_bricks(MapIn M, OccDev P, VoxelGeom G, unsigned char* __restrict__ flag) {
  const int c = blockIdx.x, p0 = M.start[c], n = M.start[c + 1] - p0;
  float R[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) R[k] = M.pose[12 * (size_t)c + k];
  long long Qo[3]; bool org_far;
  if (!occ_origin(R, P, Qo, org_far)) return;
  for (int i = blockIdx.y * 256 + threadIdx.x; i < n; i += gridDim.y * 256) {
    OccRay r;
    if (occ_ray(M, R, P, Qo, org_far, p0 + i, r) != OCC_RAY) continue;
    size_t at = ~(size_t)0;
    occ_walk(r, [&](int cx, int cy, int cz, bool) {
      const size_t b = occ_brick(G, cx, cy, cz);
      if (b != at) { flag[b] = 1; at = b; }
    });
  }
}
struct OccBrickPred {  // touched bricks -> their ascending list (at most cap entries are written) and the brick -> slot table
  const unsigned char* flag; int* list; int* slot; int cap;
  __device__ bool keep(int i) const { return flag[i]; }
  __device__ void put(int pos, int i) const { if (pos < cap) list[pos] = i; slot[i] = pos; }
};
// pass 2: one int32 atomic add per visited cell; the slot of the current brick stays in a register until the brick changes.
// steps: the cells visited, one add per wave
__global__ __launch_bounds__(256) void k_occ_accumulate(MapIn M, OccDev P, VoxelGeom G, const int* __restrict__ slot, int* __restrict__ hits,
                                                       int* __restrict__ misses, unsigned long long* __restrict__ steps) {
  const int c = blockIdx.x, p0 = M.start[c], n = M.start[c + 1] - p0;
  float R[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) R[k] = M.pose[12 * (size_t)c + k];
  long long Qo[3]; bool org_far;
  if (!occ_origin(R, P, Qo, org_far)) return;
  long long mine = 0;
  for (int i = blockIdx.y * 256 + threadIdx.x; i < n; i += gridDim.y * 256) {
    OccRay r;
    if (occ_ray(M, R, P, Qo, org_far, p0 + i, r) != OCC_RAY) continue;
    size_t at = ~(size_t)0, base = 0;
    const bool cut = r.cut;
    mine += occ_walk(r, [&](int cx, int cy, int cz, bool last) {
      const size_t b = occ_brick(G, cx, cy, cz);
      if (b != at) { base = (size_t)slot[b] * 512; at = b; }
      const size_t v = base + (size_t)((cx & 7) | ((cy & 7) << 3) | ((cz & 7) << 6));
      atomicAdd(last && !cut ? &hits[v] : &misses[v], 1);
    });
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(steps, (unsigned long long)mine);
}
struct OccLog { float l_hit, l_miss, l_min, l_max, l_occ; };
__device__ __forceinline__ float occ_logodds(const OccLog& L, int h, int m) {
  const float a = (float)h * L.l_hit, b = (float)m * L.l_miss;
  return fminf(fmaxf(a + b, L.l_min), L.l_max);
}
struct OccCellPred {   // known cells that pass emit (0 all, 1 occupied, 2 free) -> their ascending list (out may be NULL: count only)
  const int* hits; const int* misses; OccLog L; int emit; int* out; int max_out;
  __device__ bool keep(int i) const {
    const int h = hits[i], m = misses[i];
    if (h + m == 0) return false;
    if (emit == 0) return true;
    return (occ_logodds(L, h, m) >= L.l_occ) == (emit == 1);
  }
  __device__ void put(int pos, int i) const { if (pos < max_out) out[pos] = i; }
};
// pass 3: one record per kept cell
__global__ __launch_bounds__(256) void k_occ_emit(const int* __restrict__ list, int m, const int* __restrict__ bricks, VoxelGeom G, int divx, int divy,
                                                 const int* __restrict__ hits, const int* __restrict__ misses, OccLog L, int* __restrict__ out_cell,
                                                 int* __restrict__ out_hits, int* __restrict__ out_misses, float* __restrict__ out_logodds) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= m) return;
  const int v = list[k], l = v & 511, b = bricks[v >> 9];
  const int bx = b % divx + G.minb[0], by = (b / divx) % divy + G.minb[1], bz = b / divx / divy + G.minb[2];
  out_cell[3 * (size_t)k] = bx * 8 + (l & 7); out_cell[3 * (size_t)k + 1] = by * 8 + ((l >> 3) & 7); out_cell[3 * (size_t)k + 2] = bz * 8 + (l >> 6);
  out_hits[k] = hits[v]; out_misses[k] = misses[v];
  out_logodds[k] = occ_logodds(L, hits[v], misses[v]);
}
// ---- occupancy map by scans (sslam_seg_occupancy_map_scans in include/sslam.h; OctoMap's insertPointCloud [UPSTREAM]): passes 0, 1 and the
// compactions are the ray entry's.  Pass 2 runs per chunk of kOccScanW consecutive clouds: k_occ_scan_mark sets bit (cloud - base) of a
// cell's hit or miss mask, k_occ_scan_fold applies the set bits in ascending order -- the clouds' order -- to the cell's state and clears
// the masks.  Per cell of a touched brick: hits, misses, log-odds (12 B) and two 64-bit masks (16 B), 28 B.
constexpr int kOccScanW = 64;                 // clouds per chunk = bits of a mask word
typedef unsigned long long OccMask;
static_assert(kOccScanW == 8 * sizeof(OccMask), "one mask bit per cloud of a chunk");
// The two measured alternatives (DESIGN.md section 4 has the figures), each a compile-time switch so that the measurement can be repeated:
// 0 here issues the atomic OR of every visited cell without looking first; 1 below folds every cell of every touched brick in every chunk.
#ifndef SSLAM_OCC_SCAN_LOAD_FIRST
#define SSLAM_OCC_SCAN_LOAD_FIRST 1
#endif
#ifndef SSLAM_OCC_SCAN_FOLD_ALL
#define SSLAM_OCC_SCAN_FOLD_ALL 0
#endif
// the grid of k_occ_accumulate over the clouds base .. base + gridDim.x - 1 (gridDim.x <= kOccScanW).  A plain load comes first and the
// atomic only when the bit is still clear: thousands of rays of a cloud share the cells near its origin, and a stale load or a lost race
// only repeats an idempotent OR.  touched[slot] = tag (the chunk's number + 1) tells the fold which bricks this chunk entered; it is never
// cleared.  counts[0]: the cells visited, counts[1]: the atomics issued, one add per wave each.
__global__ __launch_bounds__(256) void k_occ_scan_mark(MapIn M, OccDev P, VoxelGeom G, const int* __restrict__ slot, int base, int tag, OccMask* hmask,
                                                      OccMask* mmask, int* touched, unsigned long long* __restrict__ counts) {
  const int c = base + blockIdx.x, p0 = M.start[c], n = M.start[c + 1] - p0;
  float R[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) R[k] = M.pose[12 * (size_t)c + k];
  long long Qo[3]; bool org_far;
  if (!occ_origin(R, P, Qo, org_far)) return;
  const OccMask bit = (OccMask)1 << blockIdx.x;
  long long marks = 0, issued = 0;
  for (int i = blockIdx.y * 256 + threadIdx.x; i < n; i += gridDim.y * 256) {
    OccRay r;
    if (occ_ray(M, R, P, Qo, org_far, p0 + i, r) != OCC_RAY) continue;
    size_t at = ~(size_t)0, cell0 = 0;
    const bool cut = r.cut;
    marks += occ_walk(r, [&](int cx, int cy, int cz, bool last) {
      const size_t b = occ_brick(G, cx, cy, cz);
      if (b != at) {
        const int sl = slot[b];
        if (touched[sl] != tag) touched[sl] = tag;
        cell0 = (size_t)sl * 512; at = b;
      }
      OccMask* w = (last && !cut ? hmask : mmask) + (cell0 + (size_t)((cx & 7) | ((cy & 7) << 3) | ((cz & 7) << 6)));
      if (!SSLAM_OCC_SCAN_LOAD_FIRST || !(*w & bit)) { atomicOr(w, bit); ++issued; }
    });
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { marks += __shfl_down(marks, o, 64); issued += __shfl_down(issued, o, 64); }
  if ((threadIdx.x & 63) == 0 && marks) { atomicAdd(&counts[0], (unsigned long long)marks); atomicAdd(&counts[1], (unsigned long long)issued); }
}
// one thread per cell of the touched bricks; a workgroup lies inside one brick (512 cells) and leaves at once when the chunk did not enter
// it (touched == NULL: every brick is read).  The set bits of hit | miss in ascending order, a hit overriding a miss:
// lo = fminf(fmaxf(lo + l, l_min), l_max), the sum rounded to float.  No atomics: a thread owns its cell.  (A first form counted the
// updates here, one atomic add per wave into one word: half a million waves on one address took 4 ms where the tables take 0.3 --
// DESIGN.md section 4; k_occ_scan_updates counts them once, at the end.)
__global__ __launch_bounds__(256) void k_occ_scan_fold(int ncell, const int* __restrict__ touched, int tag, OccMask* __restrict__ hmask,
                                                      OccMask* __restrict__ mmask, int* __restrict__ hits, int* __restrict__ misses,
                                                      float* __restrict__ logodds, OccLog L) {
  if (touched && touched[blockIdx.x >> 1] != tag) return;
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= ncell) return;
  const OccMask h = hmask[v], m = mmask[v] & ~h;
  OccMask left = h | m;
  if (!left) return;
  float lo = logodds[v];
  while (left) {
    const OccMask low = left & (~left + 1);
    lo = fminf(fmaxf(lo + ((h & low) ? L.l_hit : L.l_miss), L.l_min), L.l_max);
    left ^= low;
  }
  logodds[v] = lo;
  if (h) hits[v] += __popcll(h);
  if (m) misses[v] += __popcll(m);
  hmask[v] = 0; mmask[v] = 0;
}
// n_steps of the scan entry, the sum of hits + misses over the cells of the touched bricks: at most 1024 workgroups, one add each
__global__ __launch_bounds__(256) void k_occ_scan_updates(int ncell, const int* __restrict__ hits, const int* __restrict__ misses,
                                                         unsigned long long* __restrict__ updates) {
  __shared__ long long red[4];
  long long mine = 0;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < ncell; v += gridDim.x * 256) mine += hits[v] + misses[v];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0 && red[0] + red[1] + red[2] + red[3]) atomicAdd(updates, (unsigned long long)(red[0] + red[1] + red[2] + red[3]));
}
struct OccScanCellPred {   // OccCellPred over the stored, sequential log-odds
  const int* hits; const int* misses; const float* logodds; float l_occ; int emit; int* out; int max_out;
  __device__ bool keep(int i) const {
    if (hits[i] + misses[i] == 0) return false;
    if (emit == 0) return true;
    return (logodds[i] >= l_occ) == (emit == 1);
  }
  __device__ void put(int pos, int i) const { if (pos < max_out) out[pos] = i; }
};
__global__ __launch_bounds__(256) void k_occ_scan_emit(const int* __restrict__ list, int m, const int* __restrict__ bricks, VoxelGeom G, int divx, int divy,
                                                      const int* __restrict__ hits, const int* __restrict__ misses, const float* __restrict__ logodds,
                                                      int* __restrict__ out_cell, int* __restrict__ out_hits, int* __restrict__ out_misses,
                                                      float* __restrict__ out_logodds) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= m) return;
  const int v = list[k], l = v & 511, b = bricks[v >> 9];
  const int bx = b % divx + G.minb[0], by = (b / divx) % divy + G.minb[1], bz = b / divx / divy + G.minb[2];
  out_cell[3 * (size_t)k] = bx * 8 + (l & 7); out_cell[3 * (size_t)k + 1] = by * 8 + ((l >> 3) & 7); out_cell[3 * (size_t)k + 2] = bz * 8 + (l >> 6);
  out_hits[k] = hits[v]; out_misses[k] = misses[v];
  out_logodds[k] = logodds[v];
}
// pcl::StatisticalOutlierRemoval (meanK 50, plane_segmentation.cpp:583-605): mean distance of every point to its k nearest
// neighbours, exact (brute force): candidates stream through LDS tiles, every thread keeps the k + 1 smallest squared distances of
// its query in an LDS column (replace-the-maximum; after the first tiles almost every candidate is rejected by one compare)
constexpr int kSorMaxK = 64;
__global__ __launch_bounds__(128) void k_sor_mean_distance(const float* __restrict__ pts, int n, int k, float* __restrict__ mean_dist) {
  extern __shared__ float sm[];
  float* tile = sm;                         // [128][3]
  float* best = sm + 128 * 3;               // [k + 1][128]
  const int i = blockIdx.x * 128 + threadIdx.x, tid = threadIdx.x;
  const bool valid_i = i < n;
  float qx = 0, qy = 0, qz = 0;
  bool fin = false;
  if (valid_i) { qx = pts[3 * (size_t)i]; qy = pts[3 * (size_t)i + 1]; qz = pts[3 * (size_t)i + 2]; fin = isfinite(qx) && isfinite(qy) && isfinite(qz); }
  const int K = k + 1;
  const float inf = __int_as_float(0x7f800000);   // the sentinel: a squared distance that overflows is +inf as well and stands as such
  for (int j = 0; j < K; ++j) best[j * 128 + tid] = inf;
  float cur_max = inf;
  int arg_max = 0;
  for (int t0 = 0; t0 < n; t0 += 128) {
    __syncthreads();
    const int c = t0 + tid;
    tile[tid * 3] = c < n ? pts[3 * (size_t)c] : __int_as_float(0x7fc00000);
    tile[tid * 3 + 1] = c < n ? pts[3 * (size_t)c + 1] : __int_as_float(0x7fc00000);
    tile[tid * 3 + 2] = c < n ? pts[3 * (size_t)c + 2] : __int_as_float(0x7fc00000);
    __syncthreads();
    if (!fin) continue;
    const int m = min(128, n - t0);
    for (int j = 0; j < m; ++j) {
      const float dx = qx - tile[j * 3], dy = qy - tile[j * 3 + 1], dz = qz - tile[j * 3 + 2];
      const float d = (dx * dx + dy * dy) + dz * dz;      // flann::L2_Simple<float>
      if (d < cur_max) {                                   // NaN candidates fail the compare
        best[arg_max * 128 + tid] = d;
        cur_max = best[tid]; arg_max = 0;
        for (int q = 1; q < K; ++q) { const float v = best[q * 128 + tid]; if (v > cur_max) { cur_max = v; arg_max = q; } }
      }
    }
  }
  if (!valid_i) return;
  if (!fin) { mean_dist[i] = -1.0f; return; }              // not a finite point: takes no part (marked for the host)
  // ascending insertion sort of the k + 1 values, then the sum of the square roots of entries 1..k in that order (entry 0 is the point itself)
  for (int a = 1; a < K; ++a) {
    const float v = best[a * 128 + tid];
    int b = a - 1;
    while (b >= 0 && best[b * 128 + tid] > v) { best[(b + 1) * 128 + tid] = best[b * 128 + tid]; --b; }
    best[(b + 1) * 128 + tid] = v;
  }
  double sum = 0;
  for (int a = 1; a < K; ++a) sum += (double)sqrtf(best[a * 128 + tid]);
  mean_dist[i] = (float)(sum / (double)k);
}

// ---- fitness score of cloud pairs (hdl_graph_slam's InformationMatrixCalculator::calc_fitness_score; stubbed in the reference,
// information_matrix_calculator.cpp:37): exact nearest neighbour of every transformed source point among the target points ----------
// One workgroup per item = (pair, block of kNnQ source points, chunk of target points); all pairs of a call in one launch.  A thread
// keeps kNnQpt transformed queries in registers; the targets of the chunk stream through LDS kNnTile at a time as padded 16-byte
// points, and every lane reads the SAME tile address (one ds_read_b128 per target, an LDS broadcast) for kNnQpt distance evaluations
// of ~11 VALU operations each: the loop is VALU bound.  The queries of a thread are held two to a register pair, so that the three
// differences, three products and two sums of TWO queries go through packed instructions (v_pk_add_f32 / v_pk_mul_f32, the target
// coordinate broadcast to both halves): 7.4 instructions per evaluation instead of 9.5, the same IEEE operations in the same order.
// The next tile's global load is issued before the current tile is consumed.
// Ascending scan with a strict `<`: the lowest index among equal distances; a non-finite target is staged as NaN and fails every
// compare, a non-finite (or out-of-range) query is NaN and never finds anything.  The chunks of a pair meet in a 64-bit atomicMin on
// (bits of d2 << 32 | target index): non-negative floats order like their bit patterns, so the minimum is exact, independent of the
// arrival order, and keeps the lowest-index rule -- bitwise what the unsplit scan gives.  `best` starts as all ones (no neighbour).
constexpr int kNnThreads = 256, kNnQpt = 4, kNnQ = kNnThreads * kNnQpt, kNnTile = 256, kNnSeg = 256;
static_assert(kNnTile == kNnThreads, "a thread stages one target point per tile");
static_assert(kNnQpt % 2 == 0, "queries are held in pairs");
typedef float NnF2 __attribute__((ext_vector_type(2)));
static_assert(kNnSeg == 256, "k_nn_finish adds the four waves of a run in order");
struct NnPair { int t0, nt, s0, ns; long long qoff; float R[9], t[3]; double max_range; };   // point ranges in xyz; qoff: first entry of the pair in best / nn_*
struct NnItem { int pair, qblock, c0, c1; };   // targets [c0, c1) of the pair's target cloud
struct NnSeg { int pair, seg; };               // source points [seg * kNnSeg, +kNnSeg) of the pair
__global__ __launch_bounds__(kNnThreads) void k_nn_pairs(const float* __restrict__ xyz, const NnPair* __restrict__ pairs, const NnItem* __restrict__ items,
                                                         unsigned long long* __restrict__ best) {
  __shared__ float4 tile[kNnTile];
  const NnItem it = items[blockIdx.x];
  const NnPair P = pairs[it.pair];
  const int tid = threadIdx.x, ns = P.ns, nt_c = it.c1 - it.c0;
  const float nanf_ = __int_as_float(0x7fc00000);
  NnF2 qx[kNnQpt / 2], qy[kNnQpt / 2], qz[kNnQpt / 2], bd[kNnQpt / 2];   // query k = component k % 2 of pair k / 2
  int bi[kNnQpt];
#pragma unroll
  for (int k = 0; k < kNnQpt; ++k) {
    const int i = it.qblock * kNnQ + k * kNnThreads + tid;
    float tx = nanf_, ty = nanf_, tz = nanf_;
    bi[k] = -1;
    if (i < ns) {
      const float* p = xyz + 3 * (size_t)(P.s0 + i);
      const float x = p[0], y = p[1], z = p[2];
      if (isfinite(x) && isfinite(y) && isfinite(z)) {
        tx = ((P.R[0] * x + P.R[1] * y) + P.R[2] * z) + P.t[0];
        ty = ((P.R[3] * x + P.R[4] * y) + P.R[5] * z) + P.t[1];
        tz = ((P.R[6] * x + P.R[7] * y) + P.R[8] * z) + P.t[2];
      }
    }
    qx[k / 2][k % 2] = tx; qy[k / 2][k % 2] = ty; qz[k / 2][k % 2] = tz;
    bd[k / 2][k % 2] = __int_as_float(0x7f800000);
  }
  auto stage = [&](int j) {   // target j of the chunk as a padded point; NaN when it is past the chunk or not finite
    float4 c = make_float4(nanf_, nanf_, nanf_, 0.0f);
    if (j < nt_c) {
      const float* p = xyz + 3 * (size_t)(P.t0 + it.c0 + j);
      const float x = p[0], y = p[1], z = p[2];
      if (isfinite(x) && isfinite(y) && isfinite(z)) { c.x = x; c.y = y; c.z = z; }
    }
    return c;
  };
  float4 nxt = stage(tid);
  for (int b = 0; b < nt_c; b += kNnTile) {
    __syncthreads();          // the previous tile has been consumed
    tile[tid] = nxt;
    __syncthreads();
    nxt = stage(b + kNnTile + tid);
    const int m = min(kNnTile, nt_c - b), base = it.c0 + b;
#pragma unroll 4
    for (int j = 0; j < m; ++j) {
      const float4 c = tile[j];
#pragma unroll
      for (int h = 0; h < kNnQpt / 2; ++h) {
        const NnF2 dx = qx[h] - c.x, dy = qy[h] - c.y, dz = qz[h] - c.z;
        const NnF2 d = (dx * dx + dy * dy) + dz * dz;       // flann::L2_Simple<float>, two queries at a time
        if (d.x < bd[h].x) { bd[h].x = d.x; bi[2 * h] = base + j; }
        if (d.y < bd[h].y) { bd[h].y = d.y; bi[2 * h + 1] = base + j; }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kNnQpt; ++k) {
    const int i = it.qblock * kNnQ + k * kNnThreads + tid;
    if (i < ns && bi[k] >= 0)
      atomicMin(&best[P.qoff + i], ((unsigned long long)__float_as_uint(bd[k / 2][k % 2]) << 32) | (unsigned long long)(unsigned)bi[k]);
  }
}
// best -> (index, d2) per source point, and per run of kNnSeg consecutive source points of a pair the sum of the accepted (double)d2 and
// their number.  The sum's order is fixed by the point index alone: the shuffle tree of a wave over its 64 consecutive points, the four
// waves of the run in order; the host adds the runs of a pair in ascending order.
__global__ __launch_bounds__(kNnSeg) void k_nn_finish(const NnPair* __restrict__ pairs, const NnSeg* __restrict__ segs, const unsigned long long* __restrict__ best,
                                                     int* __restrict__ nn_index, float* __restrict__ nn_d2, double* __restrict__ part_sum, int* __restrict__ part_used) {
  __shared__ double red_v[kNnSeg / 64];
  __shared__ int red_u[kNnSeg / 64];
  const NnSeg sg = segs[blockIdx.x];
  const NnPair P = pairs[sg.pair];
  const int i = sg.seg * kNnSeg + threadIdx.x;
  double v = 0.0;
  int u = 0;
  if (i < P.ns) {
    const unsigned long long key = best[P.qoff + i];
    int idx = -1;
    float d = -1.0f;
    if (key != ~0ull) {
      idx = (int)(unsigned)(key & 0xffffffffull);
      d = __uint_as_float((unsigned)(key >> 32));
      if ((double)d <= P.max_range) { v = (double)d; u = 1; }
    }
    nn_index[P.qoff + i] = idx;
    nn_d2[P.qoff + i] = d;
  }
  for (int off = 32; off > 0; off >>= 1) { v += __shfl_down(v, off, 64); u += __shfl_down(u, off, 64); }
  if ((threadIdx.x & 63) == 0) { red_v[threadIdx.x >> 6] = v; red_u[threadIdx.x >> 6] = u; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part_sum[blockIdx.x] = ((red_v[0] + red_v[1]) + red_v[2]) + red_v[3];
    part_used[blockIdx.x] = ((red_u[0] + red_u[1]) + red_u[2]) + red_u[3];
  }
}

// ---- scan matching: nearest-neighbour ICP of cloud pairs (hdl_graph_slam's LoopDetector::matching with pcl::IterativeClosestPoint
// [UPSTREAM]; the reference has no scan matcher) ----------------------------------------------------------------------------------
// One iteration of ALL pairs is  reset best -> k_nn_pairs -> k_reg_sums -> k_reg_step  on the handle's stream, no host round trip:
// k_nn_pairs reads R, t from the device's pair table, and k_reg_step writes the float casts of the new estimate back into it.
//   k_reg_sums  one workgroup per run of kNnSeg consecutive source points of a pair (the NnSeg table of k_nn_finish): a thread unpacks
//               `best` for its point and, if the correspondence is accepted ((double)d2 <= max_range), loads the ORIGINAL source point p
//               (coalesced: the run's 3 * 256 floats are contiguous) and its target q (a gather: 12 bytes wherever the neighbour lies)
//               and forms, in double, sum p, sum q, sum p q^T and the count.  The products of two widened floats are exact.  Reduced
//               by block_sum4, the tree of k_nn_finish: the shuffle tree of a wave over its 64 consecutive points, the four waves in order.
//   k_reg_step  one wave per pair: lanes 0..15 add the run records in ascending run order, lane 0 solves the absolute orientation
//               problem (horn_rigid, csrc/sslam_math.hpp) and applies the status and convergence rules.
// The order of every sum is fixed by the point index alone.  A finished pair (converged, or fewer than 3 correspondences) is frozen by
// its `done` flag: its runs leave k_reg_sums at once and its state and pair-table entry are never written again; it still rides through
// k_nn_pairs, whose instruction stream is the fitness pass's.
constexpr int kRegSums = 16;   // sum p (3), sum q (3), sum p q^T (9, row-major: p's coordinate is the row), count
struct RegState { double T[12]; int iterations, converged, status, done; };
__global__ __launch_bounds__(kNnSeg) void k_reg_sums(const float* __restrict__ xyz, const NnPair* __restrict__ pairs, const NnSeg* __restrict__ segs,
                                                    const unsigned long long* __restrict__ best, const RegState* __restrict__ st,
                                                    double* __restrict__ part) {
  __shared__ double red[kNnSeg / 64][kRegSums];
  const NnSeg sg = segs[blockIdx.x];
  if (st[sg.pair].done) return;          // the same for the whole workgroup
  const NnPair P = pairs[sg.pair];
  const int tid = threadIdx.x, i = sg.seg * kNnSeg + tid;
  double a[kRegSums];
#pragma unroll
  for (int k = 0; k < kRegSums; ++k) a[k] = 0.0;
  if (i < P.ns) {
    const unsigned long long key = best[P.qoff + i];
    if (key != ~0ull && (double)__uint_as_float((unsigned)(key >> 32)) <= P.max_range) {
      const int j = (int)(unsigned)(key & 0xffffffffull);   // < P.nt: k_nn_pairs only ever writes indices of the pair's target cloud
      const float* ps = xyz + 3 * (size_t)(P.s0 + i);
      const float* qt = xyz + 3 * (size_t)(P.t0 + j);
      const double p[3] = {(double)ps[0], (double)ps[1], (double)ps[2]}, q[3] = {(double)qt[0], (double)qt[1], (double)qt[2]};
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        a[r] = p[r]; a[3 + r] = q[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) a[6 + 3 * r + c] = p[r] * q[c];
      }
      a[15] = 1.0;
    }
  }
  block_sum4(a, red, part + (size_t)blockIdx.x * kRegSums);
}
__global__ __launch_bounds__(64) void k_reg_step(const int* __restrict__ seg0, const double* __restrict__ part, double epsilon, NnPair* __restrict__ pairs,
                                                 RegState* __restrict__ st, int* __restrict__ live) {
  __shared__ double sums[kRegSums];
  const int p = blockIdx.x, tid = threadIdx.x;
  if (st[p].done) return;
  if (tid < kRegSums) {
    double v = 0.0;
    for (int r = seg0[p]; r < seg0[p + 1]; ++r) v += part[(size_t)r * kRegSums + tid];   // ascending run order
    sums[tid] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  if (sums[15] < 3.0) {                  // fewer than 3 correspondences: T stays as it stood before this pass
    st[p].status = SSLAM_ERR_NUMERIC;
    st[p].done = 1;
    atomicSub(live, 1);
    return;
  }
  double Tn[12], moved = 0.0;            // sums of finite floats and their pairwise products cannot overflow a double: Tn is finite
  horn_rigid(sums[15], sums[0], sums[1], sums[2], sums[3], sums[4], sums[5], sums[6], sums[7], sums[8], sums[9], sums[10], sums[11], sums[12],
             sums[13], sums[14], Tn);
#pragma unroll
  for (int k = 0; k < 12; ++k) moved = fmax(moved, fabs(Tn[k] - st[p].T[k]));
#pragma unroll
  for (int k = 0; k < 12; ++k) st[p].T[k] = Tn[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) pairs[p].R[k] = (float)Tn[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) pairs[p].t[k] = (float)Tn[9 + k];
  st[p].iterations += 1;
  if (moved <= epsilon) {
    st[p].converged = 1;
    st[p].done = 1;
    atomicSub(live, 1);
  }
}

// ---- generalized ICP (fast_gicp / pcl::GeneralizedIterativeClosestPoint [UPSTREAM]: hdl_graph_slam's registration_method GICP / FAST_GICP) ----
// k_knn_cov: the covariance of every point's k nearest neighbours inside its own cloud, regularised to a plane (gicp_plane_covariance).
// One workgroup per block of kKnnThreads consecutive query points of ONE cloud (the KnnBlock table), one thread per query.  The cloud
// streams through LDS kKnnThreads points at a time; every thread keeps the k smallest (d2, index) of its query in two LDS columns
// (replace-the-maximum, as k_sor_mean_distance keeps its distances).  Candidates arrive in ascending index, so a candidate enters only
// with a strictly smaller d2 than the column's maximum or into an empty slot (+inf, INT_MAX): the set is the k smallest by (d2, index)
// whatever the tile or block size.  The columns are then sorted ascending; mean and covariance run in double in that order.
constexpr int kKnnThreads = 128;
static_assert(SSLAM_ERR_INVALID == -1, "gicp_check_params (csrc/sslam_common.hpp) returns it by value");
static_assert(kKnnThreads * (3 * sizeof(float) + kGicpMaxK * (sizeof(float) + sizeof(int))) <= 64 * 1024, "the columns of the largest k fit the LDS of a workgroup");
struct KnnBlock { int c0, n, q0; };   // first point of the cloud in xyz, its points, the block's first query inside the cloud
__global__ __launch_bounds__(kKnnThreads) void k_knn_cov(const float* __restrict__ xyz, const KnnBlock* __restrict__ blocks, int k, double eps,
                                                        double* __restrict__ cov, int* __restrict__ knn) {
  extern __shared__ float sm[];
  float* tile = sm;                                   // [kKnnThreads][3]
  float* bd = sm + kKnnThreads * 3;                   // [k][kKnnThreads]
  int* bi = (int*)(bd + k * kKnnThreads);             // [k][kKnnThreads]
  const KnnBlock B = blocks[blockIdx.x];
  const int tid = threadIdx.x, i = B.q0 + tid;
  const float* pts = xyz + 3 * (size_t)B.c0;
  const bool valid_i = i < B.n;
  float qx = 0, qy = 0, qz = 0;
  bool fin = false;
  if (valid_i) { qx = pts[3 * (size_t)i]; qy = pts[3 * (size_t)i + 1]; qz = pts[3 * (size_t)i + 2]; fin = isfinite(qx) && isfinite(qy) && isfinite(qz); }
  const float inf = __int_as_float(0x7f800000), nanf_ = __int_as_float(0x7fc00000);
  for (int j = 0; j < k; ++j) { bd[j * kKnnThreads + tid] = inf; bi[j * kKnnThreads + tid] = INT_MAX; }
  float max_d = inf;
  int max_i = INT_MAX, arg_max = 0;
  for (int t0 = 0; t0 < B.n; t0 += kKnnThreads) {
    __syncthreads();
    const int c = t0 + tid;
    float cx = nanf_, cy = nanf_, cz = nanf_;
    if (c < B.n) {
      const float x = pts[3 * (size_t)c], y = pts[3 * (size_t)c + 1], z = pts[3 * (size_t)c + 2];
      if (isfinite(x) && isfinite(y) && isfinite(z)) { cx = x; cy = y; cz = z; }
    }
    tile[tid * 3] = cx; tile[tid * 3 + 1] = cy; tile[tid * 3 + 2] = cz;
    __syncthreads();
    if (!fin) continue;
    const int m = min(kKnnThreads, B.n - t0);
    for (int j = 0; j < m; ++j) {
      const float dx = qx - tile[j * 3], dy = qy - tile[j * 3 + 1], dz = qz - tile[j * 3 + 2];
      const float d = (dx * dx + dy * dy) + dz * dz;
      if (d < max_d || (d == max_d && t0 + j < max_i)) {    // a NaN candidate (not a finite point) fails both
        bd[arg_max * kKnnThreads + tid] = d; bi[arg_max * kKnnThreads + tid] = t0 + j;
        max_d = bd[tid]; max_i = bi[tid]; arg_max = 0;
        for (int q = 1; q < k; ++q) {
          const float v = bd[q * kKnnThreads + tid];
          const int w = bi[q * kKnnThreads + tid];
          if (v > max_d || (v == max_d && w > max_i)) { max_d = v; max_i = w; arg_max = q; }
        }
      }
    }
  }
  if (!valid_i) return;
  double* out = cov + 6 * ((size_t)B.c0 + i);
  int* kout = knn ? knn + (size_t)k * ((size_t)B.c0 + i) : nullptr;
  if (!fin) {
#pragma unroll
    for (int q = 0; q < 6; ++q) out[q] = 0.0;
    if (kout) for (int q = 0; q < k; ++q) kout[q] = -1;
    return;
  }
  for (int a = 1; a < k; ++a) {          // ascending insertion sort by (d2, index); the empty slots end up last
    const float v = bd[a * kKnnThreads + tid];
    const int w = bi[a * kKnnThreads + tid];
    int b = a - 1;
    while (b >= 0 && (bd[b * kKnnThreads + tid] > v || (bd[b * kKnnThreads + tid] == v && bi[b * kKnnThreads + tid] > w))) {
      bd[(b + 1) * kKnnThreads + tid] = bd[b * kKnnThreads + tid]; bi[(b + 1) * kKnnThreads + tid] = bi[b * kKnnThreads + tid]; --b;
    }
    bd[(b + 1) * kKnnThreads + tid] = v; bi[(b + 1) * kKnnThreads + tid] = w;
  }
  int m = 0;
  while (m < k && bi[m * kKnnThreads + tid] != INT_MAX) ++m;
  if (kout) for (int q = 0; q < k; ++q) kout[q] = q < m ? bi[q * kKnnThreads + tid] : -1;
  if (m < 3) { out[0] = 1.0; out[1] = 0.0; out[2] = 0.0; out[3] = 1.0; out[4] = 0.0; out[5] = 1.0; return; }
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int q = 0; q < m; ++q) {
    const float* p = pts + 3 * (size_t)bi[q * kKnnThreads + tid];
    sx += (double)p[0]; sy += (double)p[1]; sz += (double)p[2];
  }
  const double mx = sx / (double)m, my = sy / (double)m, mz = sz / (double)m;
  double C[6] = {0, 0, 0, 0, 0, 0};
  for (int q = 0; q < m; ++q) {
    const float* p = pts + 3 * (size_t)bi[q * kKnnThreads + tid];
    const double ax = (double)p[0] - mx, ay = (double)p[1] - my, az = (double)p[2] - mz;
    C[0] += ax * ax; C[1] += ax * ay; C[2] += ax * az; C[3] += ay * ay; C[4] += ay * az; C[5] += az * az;
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) C[q] /= (double)m;
  double P[6];
  gicp_plane_covariance(C, eps, P);
#pragma unroll
  for (int q = 0; q < 6; ++q) out[q] = P[q];
}
// One iteration of ALL pairs is  reset best -> k_nn_pairs -> k_gicp_sums -> k_gicp_step: the structure of the point-to-point loop above.
//   k_gicp_sums  the run table and the reduction tree of k_reg_sums; an accepted point i with its target j contributes gicp_point_sums
//                (csrc/sslam_math.hpp) at the pair's double T with the covariances of source point i and target point j: 29 sums.
//   k_gicp_step  one wave per pair: lanes 0..28 add the run records in ascending run order, lane 0 takes gicp_gn_step and applies the
//                status and convergence rules of k_reg_step.
__global__ __launch_bounds__(kNnSeg) void k_gicp_sums(const float* __restrict__ xyz, const double* __restrict__ cov, const NnPair* __restrict__ pairs,
                                                     const NnSeg* __restrict__ segs, const unsigned long long* __restrict__ best,
                                                     const RegState* __restrict__ st, double* __restrict__ part) {
  __shared__ double red[kNnSeg / 64][kIcpSums];
  const NnSeg sg = segs[blockIdx.x];
  if (st[sg.pair].done) return;          // the same for the whole workgroup
  const NnPair P = pairs[sg.pair];
  const int tid = threadIdx.x, i = sg.seg * kNnSeg + tid;
  double a[kIcpSums];
#pragma unroll
  for (int k = 0; k < kIcpSums; ++k) a[k] = 0.0;
  if (i < P.ns) {
    const unsigned long long key = best[P.qoff + i];
    if (key != ~0ull && (double)__uint_as_float((unsigned)(key >> 32)) <= P.max_range) {
      const int j = (int)(unsigned)(key & 0xffffffffull);   // < P.nt: k_nn_pairs only ever writes indices of the pair's target cloud
      const float* ps = xyz + 3 * (size_t)(P.s0 + i);
      const float* qt = xyz + 3 * (size_t)(P.t0 + j);
      const double* cs = cov + 6 * (size_t)(P.s0 + i);
      const double* ct = cov + 6 * (size_t)(P.t0 + j);
      const double p[3] = {(double)ps[0], (double)ps[1], (double)ps[2]}, q[3] = {(double)qt[0], (double)qt[1], (double)qt[2]};
      const double Cs[6] = {cs[0], cs[1], cs[2], cs[3], cs[4], cs[5]}, Ct[6] = {ct[0], ct[1], ct[2], ct[3], ct[4], ct[5]};
      double T[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) T[k] = st[sg.pair].T[k];
      gicp_point_sums(T, p, q, Cs, Ct, a);
    }
  }
  block_sum4(a, red, part + (size_t)blockIdx.x * kIcpSums);
}
__global__ __launch_bounds__(64) void k_gicp_step(const int* __restrict__ seg0, const double* __restrict__ part, double epsilon, NnPair* __restrict__ pairs,
                                                  RegState* __restrict__ st, int* __restrict__ live) {
  __shared__ double sums[kIcpSums];
  const int p = blockIdx.x, tid = threadIdx.x;
  if (st[p].done) return;
  if (tid < kIcpSums) {
    double v = 0.0;
    for (int r = seg0[p]; r < seg0[p + 1]; ++r) v += part[(size_t)r * kIcpSums + tid];   // ascending run order
    sums[tid] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  double Tn[12], moved = 0.0;
  if (!gicp_gn_step(sums, st[p].T, Tn)) {   // T stays as it stood before this pass
    st[p].status = SSLAM_ERR_NUMERIC;
    st[p].done = 1;
    atomicSub(live, 1);
    return;
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) moved = fmax(moved, fabs(Tn[k] - st[p].T[k]));
#pragma unroll
  for (int k = 0; k < 12; ++k) st[p].T[k] = Tn[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) pairs[p].R[k] = (float)Tn[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) pairs[p].t[k] = (float)Tn[9 + k];
  st[p].iterations += 1;
  if (moved <= epsilon) {
    st[p].converged = 1;
    st[p].done = 1;
    atomicSub(live, 1);
  }
}

// ---- k-means of the legacy path (plane_segmentation::computeKmeans -> cv::kmeans, plane_segmentation.cpp:524-535) -----------------
// assignment step: nearest centre in float32 (squared distance accumulated coordinate by coordinate; ties -> lowest centre), and for
// the next centre update the coordinate sums / counts per cluster and the compactness, all in 2^-20 fixed point (integer atomics)
constexpr int kKmMaxK = 16;
struct KmCenters { float c[kKmMaxK * 3]; int k, dim; };
__global__ __launch_bounds__(256) void k_kmeans_assign(const float* __restrict__ pts, int n, KmCenters C, int* __restrict__ labels,
                                                      long long* __restrict__ sums, int* __restrict__ counts, long long* __restrict__ compact) {
  __shared__ long long s_sum[kKmMaxK * 3];
  __shared__ int s_cnt[kKmMaxK];
  __shared__ long long s_cmp;
  for (int t = threadIdx.x; t < kKmMaxK * 3; t += 256) s_sum[t] = 0;
  if (threadIdx.x < kKmMaxK) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x == 0) s_cmp = 0;
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    float p[3] = {0, 0, 0};
    for (int d = 0; d < C.dim; ++d) p[d] = pts[(size_t)i * C.dim + d];
    float best = 3.402823466e+38f;
    int arg = 0;
    for (int j = 0; j < C.k; ++j) {
      float dist = 0;
      for (int d = 0; d < C.dim; ++d) { const float t = p[d] - C.c[j * 3 + d]; dist += t * t; }
      if (dist < best) { best = dist; arg = j; }
    }
    labels[i] = arg;
    for (int d = 0; d < C.dim; ++d) atomicAdd((unsigned long long*)&s_sum[arg * 3 + d], (unsigned long long)llrint((double)p[d] * 1048576.0));
    atomicAdd(&s_cnt[arg], 1);
    atomicAdd((unsigned long long*)&s_cmp, (unsigned long long)llrint((double)best * 1048576.0));
  }
  __syncthreads();
  for (int t = threadIdx.x; t < C.k * 3; t += 256) if (s_sum[t]) atomicAdd((unsigned long long*)&sums[t], (unsigned long long)s_sum[t]);
  if (threadIdx.x < C.k && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], s_cnt[threadIdx.x]);
  if (threadIdx.x == 0 && s_cmp) atomicAdd((unsigned long long*)compact, (unsigned long long)s_cmp);
}
}  // namespace seg
}  // namespace sslam

// =================================================================================================
// host side + C-ABI
// =================================================================================================
using namespace sslam;
using namespace sslam::seg;

struct sslam_seg {
  sslam_seg_params P;
  hipStream_t stream = nullptr;
  View V{};
  std::vector<BoxMeta> boxes;      // accepted boxes of the last call
  std::vector<int> box_src;        // accepted slot -> index into the caller's box array (of its frame)
  std::vector<int> box_frame;      // accepted slot -> frame of the batched call
  int last_dropped_planes = 0, last_candidate_overflow = 0, last_region_overflow = 0;
  size_t cap_pix = 0, cap_ii = 0, cap_cloud = 0, cap_box = 0;
  unsigned char* d_cloud = nullptr;
  BoxMeta* d_box = nullptr;
  double last_kernel_ms = 0, last_total_ms = 0;
  std::vector<void*> allocs;
  // a batch between its enqueue (H2D + kernels + result tables D2H, all asynchronous on `stream`) and its finish (wait + scalar
  // post-processing): what the post-processing needs from the caller's frames, copied so that only the clouds must stay alive
  struct FrameMeta { float robot_pose[6]; float cam_angle; };
  struct BoxInfo { float prob; int class_id; };
  std::vector<FrameMeta> q_frames;
  std::vector<BoxInfo> q_boxes;    // per accepted slot
  Region* q_regs = nullptr;        // pinned: the result tables come back asynchronously (a pageable target would make the enqueue wait)
  int* q_nreg = nullptr;           // [cap_q_box + 2]: region counts, then the two overflow counters
  size_t cap_q_box = 0;
  hipEvent_t q_e0 = nullptr, q_e1 = nullptr;
  bool q_e1_armed = false;         // q_e1 has been recorded behind the kernels of a batch (the peer pipeline's next batch waits for it)
  bool q_busy = false;
  std::chrono::steady_clock::time_point q_t0;
  // sslam_seg_submit_batch / _collect_batch: two pipelines (this handle and a twin with its own stream and buffers) used in turn, so
  // that the H2D copy of one batch runs under the kernels of the previous one
  // sslam_seg_ransac_boxes / _icp_boxes over the resident batch of the last blocking segment call
  unsigned char* d_rflag = nullptr;   // [pixels of the batch] inlier of its box's refined RANSAC model
  void* d_rbox = nullptr;             // RansacBox per accepted box
  void* d_icp = nullptr;              // sslam_seg_icp_boxes: [tables | per-frame state | per-box partial sums | results], grows only
  size_t cap_icp = 0;
  std::vector<char> h_icp;            // host image of the tables + state (one H2D copy per call)
  size_t cap_rflag = 0, cap_rbox = 0;
  int r_nbox = -1;                    // boxes the flags belong to (-1: no RANSAC has run on the resident batch)
  hipEvent_t f_e0 = nullptr, f_e1 = nullptr;   // sslam_seg_fitness_scores: around the kernels of the pass
  int n_cu = 0;                       // compute units of the device (sizes the target split of k_nn_pairs)
  hipEvent_t m_ev[8] = {};            // the map cloud: start / stop around each of its four passes
  double map_pass_ms[4] = {0, 0, 0, 0};
  double occ_pass_ms[4] = {0, 0, 0, 0};   // the occupancy map's four passes (it shares the map cloud's events)
  std::vector<hipEvent_t> occ_scan_ev;    // the occupancy map by scans: 2 * chunks + 1 events around its mark and fold launches, grows only
  double occ_scan_ms[2] = {0, 0};         // mark, fold: summed over the chunks of the last call
  int64_t occ_scan_counts[2] = {0, 0};    // the cells the last call's mark launches visited, the atomics they issued
  sslam_seg* twin = nullptr;
  int fifo[2] = {0, 0};            // which pipeline (0 = this, 1 = twin) holds the oldest / the newer submitted batch
  int n_inflight = 0;
  ~sslam_seg() {
    delete twin;
    if (stream) { (void)hipSetDevice(P.device); (void)hipStreamSynchronize(stream); }
    free_all();
    if (q_regs) (void)hipHostFree(q_regs);
    if (q_nreg) (void)hipHostFree(q_nreg);
    if (d_rflag) (void)hipFree(d_rflag);
    if (d_rbox) (void)hipFree(d_rbox);
    if (d_icp) (void)hipFree(d_icp);
    if (q_e0) (void)hipEventDestroy(q_e0);
    if (q_e1) (void)hipEventDestroy(q_e1);
    if (f_e0) (void)hipEventDestroy(f_e0);
    if (f_e1) (void)hipEventDestroy(f_e1);
    for (hipEvent_t e : m_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : occ_scan_ev) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }
  void free_all() {
    for (void* p : allocs) (void)hipFree(p);
    allocs.clear();
  }
};

static void host_mat4_mul(const float* A, const float* B, float* C) {
  float T[16];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      float s = 0;
      for (int k = 0; k < 4; ++k) s += A[r * 4 + k] * B[k * 4 + c];
      T[r * 4 + c] = s;
    }
  memcpy(C, T, sizeof T);
}

template <typename T>
static int seg_alloc(sslam_seg* s, size_t n, T** out) {
  void* p = nullptr;
  SSLAM_HIP_TRY(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
  s->allocs.push_back(p);
  *out = (T*)p;
  return 0;
}

// helpers of the single-cloud entry points (RANSAC plane, hull, ICP, cloud filters, fitness, registration)
namespace {
struct DevGuard {
  std::vector<void*> ptrs;
  ~DevGuard() { for (void* p : ptrs) if (p) (void)hipFree(p); }
  template <class T> int alloc(T** p, size_t count) {
    void* q = nullptr;
    SSLAM_HIP_TRY(hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
    ptrs.push_back(q); *p = (T*)q;
    return 0;
  }
};
int seg_have_device() {
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return set_error(SSLAM_ERR_NO_DEVICE, "no HIP device visible; the product has no CPU fallback");
  return 0;
}
int seg_device(sslam_seg* s) {
  int rc = seg_have_device();
  if (rc) return rc;
  SSLAM_HIP_TRY(hipSetDevice(s->P.device));
  if (!s->stream) SSLAM_HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  return 0;
}
// ordered compaction of [0, n) under `pred` on the handle's stream (k_count_if -> k_exclusive_scan -> k_write_if).  d_blk: one int per
// block of 256, d_total: one int, which keeps the number kept; with total_out the call waits and returns that number on the host too.
// wide: the scan by a whole workgroup (k_exclusive_scan_wide), for an n in the millions.
template <class Pred>
int compact_if(sslam_seg* s, Pred pred, int n, int* d_blk, int* d_total, int* total_out, bool wide = false) {
  const int nblk = (n + 255) / 256;
  hipLaunchKernelGGL(k_count_if<Pred>, dim3(nblk), dim3(256), 0, s->stream, pred, n, d_blk);
  if (wide) hipLaunchKernelGGL(k_exclusive_scan_wide, dim3(1), dim3(1024), 0, s->stream, d_blk, nblk, d_blk, d_total);
  else hipLaunchKernelGGL(k_exclusive_scan, dim3(1), dim3(64), 0, s->stream, d_blk, nblk, d_blk, d_total);
  hipLaunchKernelGGL(k_write_if<Pred>, dim3(nblk), dim3(256), 0, s->stream, pred, n, d_blk);
  SSLAM_HIP_TRY(hipGetLastError());
  if (!total_out) return 0;
  SSLAM_HIP_TRY(hipMemcpyAsync(total_out, d_total, sizeof(int), hipMemcpyDeviceToHost, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  return 0;
}
// ascending indices of the set flags -> d_out; their number -> *total_out (host)
int compact_flags(sslam_seg* s, DevGuard& g, const unsigned char* d_flag, int n, int* d_out, int max_out, int* total_out) {
  int *d_blk = nullptr, *d_total = nullptr;
  int rc;
  if ((rc = g.alloc(&d_blk, (n + 255) / 256)) || (rc = g.alloc(&d_total, 1))) return rc;
  return compact_if(s, FlagPred{d_flag, d_out, max_out}, n, d_blk, d_total, total_out);
}
}  // namespace

extern "C" {

void sslam_seg_default_params(sslam_seg_params* p) {
  if (!p) return;
  p->num_point_seg = 500; p->norm_point_thres = 5000; p->planar_area = 0.1;   // plane_segmentation.cpp:7-9
  p->max_depth_change_factor = 0.03f; p->normal_smoothing_size = 20.0f;        // :99-100
  p->angular_threshold = (float)(0.017453 * 2.0); p->distance_threshold = 0.02f;  // :140-141
  p->maximum_curvature = 0.001f;
  p->min_contour_points = 100;                                                 // :169
  p->image_width = 640; p->image_height = 480;                                 // :34-35
  p->reference_quirks = 1; p->device = 0;
}

sslam_seg* sslam_seg_create(const sslam_seg_params* p) {
  sslam_seg* s = new sslam_seg();
  if (p) s->P = *p; else sslam_seg_default_params(&s->P);
  return s;
}
void sslam_seg_destroy(sslam_seg* s) { delete s; }

// semantic_tools::transformNormalsToWorld (tools.h:18-102), float matrix chain as in the reference
int sslam_seg_transform(const sslam_seg* s, const float pose[6], float cam_pitch, float out[16]) {
  if (!pose || !out) return set_error(SSLAM_ERR_INVALID, "null argument");
  const int quirks = s ? s->P.reference_quirks : 1;
  float rxc[16] = {0}, rxr[16] = {0}, rzr[16] = {0}, T[16] = {0};
  const double roll = pose[3], pitch = pose[4], yaw = pose[5];
  const double a = -(double)cam_pitch;
  rxc[0] = 1; rxc[5] = (float)cos(a); rxc[6] = (float)-sin(a); rxc[9] = (float)sin(a); rxc[10] = (float)cos(a); rxc[15] = 1;
  rxr[0] = 1; rxr[5] = (float)cos(-1.5708); rxr[6] = (float)-sin(-1.5708); rxr[9] = (float)sin(-1.5708); rxr[10] = (float)cos(-1.5708); rxr[15] = 1;
  rzr[0] = (float)cos(-1.5708); rzr[1] = (float)-sin(-1.5708); rzr[4] = (float)sin(-1.5708); rzr[5] = (float)cos(-1.5708); rzr[10] = 1; rzr[15] = 1;
  T[0] = (float)(cos(yaw) * cos(pitch));
  T[1] = (float)(cos(yaw) * sin(pitch) * sin(roll) - sin(yaw) * cos(roll));
  T[2] = (float)(cos(yaw) * sin(pitch) * cos(roll) + sin(yaw) * (quirks ? sin(pitch) : sin(roll)));  // tools.h:80-81 (quirk B2)
  T[4] = (float)(sin(yaw) * cos(pitch));
  T[5] = (float)(sin(yaw) * sin(pitch) * sin(roll) + cos(yaw) * cos(roll));
  T[6] = (float)(sin(yaw) * sin(pitch) * cos(roll) - cos(yaw) * sin(roll));
  T[8] = (float)(-sin(pitch)); T[9] = (float)(cos(pitch) * sin(roll)); T[10] = (float)(cos(pitch) * cos(roll)); T[15] = 1;
  float M[16];
  host_mat4_mul(T, rzr, M); host_mat4_mul(M, rxr, M); host_mat4_mul(M, rxc, out);
  return 0;
}

// One or several frames in one pass: the accepted boxes of ALL frames are packed back to back into one View, so that every
// kernel launch covers 32 x F boxes (a single frame's 32 boxes leave most of the 256 CUs idle: the raster recurrences of PCL's
// algorithms run as one workgroup per box).
// The kernels that stage bands / label images take up to ~150 KiB of dynamic LDS.  The opt-in belongs to the kernel, not to a call: one
// value, set once per device under a lock (handles on several host threads would otherwise overwrite one another's smaller values).
static int seg_lds_opt_in(int device) {
  static std::mutex mu;
  static std::vector<int> done;
  std::lock_guard<std::mutex> lk(mu);
  if (std::find(done.begin(), done.end(), device) != done.end()) return 0;
  const int v = lds_optin_limit(device, 156 * 1024, 4096);
  const void* fns[] = {(const void*)k_distance_map, (const void*)k_refine, (const void*)k_integral, (const void*)k_cc_lds, (const void*)k_refine_lds,
                       (const void*)k_contour<true>};
  for (const void* f : fns) SSLAM_HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, v));
  done.push_back(device);
  return 0;
}
static int seg_enqueue(sslam_seg* s, const sslam_frame* frames, int n_frames, int width, int height, int point_step, int row_step, int ox, int oy, int oz,
                       sslam_seg* peer = nullptr) {
  if (!s || !frames) return set_error(SSLAM_ERR_INVALID, "null argument");
  if (n_frames <= 0) return set_error(SSLAM_ERR_INVALID, "n_frames %d", n_frames);
  if (s->q_busy) return set_error(SSLAM_ERR_INVALID, "the previous batch of this pipeline has not been collected");
  // the cloud layout feeds k_crop's address arithmetic (row * row_step + col * point_step + offset) unchecked from here on: every
  // read of a pixel inside the image must stay inside the row_step * height bytes that are copied to the device
  if (width <= 0 || height <= 0) return set_error(SSLAM_ERR_INVALID, "cloud of %d x %d points", width, height);
  if (point_step < 4) return set_error(SSLAM_ERR_INVALID, "point_step %d holds no float", point_step);
  if (ox < 0 || oy < 0 || oz < 0 || ox > point_step - 4 || oy > point_step - 4 || oz > point_step - 4)
    return set_error(SSLAM_ERR_INVALID, "field offsets (%d, %d, %d) outside a point of %d bytes", ox, oy, oz, point_step);
  if ((long long)row_step < (long long)width * point_step)
    return set_error(SSLAM_ERR_INVALID, "row_step %d below width * point_step = %lld", row_step, (long long)width * point_step);
  for (int f = 0; f < n_frames; ++f) {
    if (frames[f].n_boxes < 0) return set_error(SSLAM_ERR_INVALID, "frame %d: n_boxes %d", f, frames[f].n_boxes);
    if (!frames[f].cloud || (!frames[f].boxes && frames[f].n_boxes > 0)) return set_error(SSLAM_ERR_INVALID, "frame %d: null cloud or boxes", f);
  }
  { const int rc_dev = seg_device(s); if (rc_dev) return rc_dev; }
  s->q_t0 = std::chrono::steady_clock::now();
  const sslam_seg_params& P = s->P;
  // ---- host-side box filter: class whitelist (point_cloud_segmentation.h:126-130), crop bounds
  //      (plane_segmentation.cpp:34-38), minimum point count (:93-95)
  s->boxes.clear(); s->box_src.clear(); s->box_frame.clear();
  s->r_nbox = -1;
  size_t npix = 0, nii = 0;
  int maxpix = 1;
  for (int f = 0; f < n_frames; ++f)
  for (int i = 0; i < frames[f].n_boxes; ++i) {
    const sslam_box& b = frames[f].boxes[i];
    if (b.class_id < SSLAM_CLASS_CHAIR || b.class_id > SSLAM_CLASS_CAR) continue;
    if (b.height < 0 || b.width < 0 || b.tl_x < 0 || b.tl_y < 0 || (b.tl_x + b.width) > P.image_width || (b.tl_y + b.height) > P.image_height) continue;
    if (b.tl_x + b.width > width || b.tl_y + b.height > height) continue;
    const size_t n = (size_t)b.width * b.height;
    if (n == 0 || (double)n < P.norm_point_thres) continue;
    if (b.width > kBandFloats / 8 - 1) return set_error(SSLAM_ERR_UNSUPPORTED, "box wider than %d px", kBandFloats / 8 - 1);
    BoxMeta m{b.width, b.height, b.tl_x, b.tl_y, (int)npix, (int)nii, (int)s->boxes.size(), f};
    s->boxes.push_back(m); s->box_src.push_back(i); s->box_frame.push_back(f);
    if (npix + n >= ((size_t)1 << 29)) return set_error(SSLAM_ERR_UNSUPPORTED, "too many box pixels in one call (%zu): split the batch", npix + n);
    npix += n; nii += (size_t)(b.width + 1) * (b.height + 1);
    maxpix = std::max(maxpix, (int)n);
  }
  const int nb = (int)s->boxes.size();
  View& V = s->V;
  const size_t frame_bytes = (size_t)row_step * height;
  const size_t cloud_bytes = frame_bytes * n_frames;
  if (cloud_bytes > s->cap_cloud || npix > s->cap_pix || nii > s->cap_ii || (size_t)nb > s->cap_box) {
    SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
    s->free_all();
    s->cap_cloud = cloud_bytes; s->cap_pix = std::max<size_t>(npix, 1); s->cap_ii = std::max<size_t>(nii, 1); s->cap_box = std::max(nb, 1);
    int rc;
    if ((rc = seg_alloc(s, s->cap_cloud, &s->d_cloud))) return rc;
    if ((rc = seg_alloc(s, s->cap_box, &s->d_box))) return rc;
    if ((rc = seg_alloc(s, s->cap_pix * 3, &V.pts))) return rc;
    if ((rc = seg_alloc(s, s->cap_pix, &V.dm))) return rc;
    if ((rc = seg_alloc(s, s->cap_pix * 4, &V.nrm))) return rc;
    if ((rc = seg_alloc(s, s->cap_pix, &V.pd))) return rc;
    if ((rc = seg_alloc(s, s->cap_pix, &V.lab))) return rc;
    if ((rc = seg_alloc(s, s->cap_pix, &V.cnt))) return rc;
    if ((rc = seg_alloc(s, s->cap_pix, &V.l2m))) return rc;
    if ((rc = seg_alloc(s, s->cap_pix, &V.code))) return rc;
    if ((rc = seg_alloc(s, s->cap_ii * 10, &V.ii))) return rc;
    if ((rc = seg_alloc(s, s->cap_box * kMaxRegions, &V.reg))) return rc;
    if ((rc = seg_alloc(s, s->cap_box, &V.nreg))) return rc;
    if ((rc = seg_alloc(s, s->cap_pix * 4, &V.contour))) return rc;
    if ((rc = seg_alloc(s, s->cap_box, &V.ccount))) return rc;
    if ((rc = seg_alloc(s, (size_t)8, &V.overflow))) return rc;   // [2] overflow counters (+ spare)
  }
  V.nbox = nb; V.npix_total = (int)npix; V.maxpix = maxpix;
  V.box = s->d_box; V.cloud = s->d_cloud; V.cloud_stride = frame_bytes;
  V.point_step = point_step; V.row_step = row_step; V.ox = ox; V.oy = oy; V.oz = oz;
  V.mdcf = P.max_depth_change_factor; V.smoothing = P.normal_smoothing_size;
  V.ang_thr_cos = cosf(P.angular_threshold); V.dist_thr = P.distance_threshold; V.max_curv = P.maximum_curvature;
  V.min_inliers = (unsigned)P.num_point_seg;
  V.refine_bh = nb > 512 ? 24 : 64;
  s->q_frames.resize(n_frames);
  for (int f = 0; f < n_frames; ++f) { memcpy(s->q_frames[f].robot_pose, frames[f].robot_pose, sizeof(float) * 6); s->q_frames[f].cam_angle = frames[f].cam_angle; }
  s->q_boxes.resize(nb);
  for (int bi = 0; bi < nb; ++bi) { const sslam_box& sb = frames[s->box_frame[bi]].boxes[s->box_src[bi]]; s->q_boxes[bi] = {sb.prob, sb.class_id}; }
  if ((size_t)nb > s->cap_q_box || !s->q_regs) {
    if (s->q_regs) (void)hipHostFree(s->q_regs);
    if (s->q_nreg) (void)hipHostFree(s->q_nreg);
    s->q_regs = nullptr; s->q_nreg = nullptr;
    s->cap_q_box = std::max<size_t>(nb, 1);
    SSLAM_HIP_TRY(hipHostMalloc((void**)&s->q_regs, s->cap_q_box * kMaxRegions * sizeof(Region), hipHostMallocDefault));
    SSLAM_HIP_TRY(hipHostMalloc((void**)&s->q_nreg, (s->cap_q_box + 2) * sizeof(int), hipHostMallocDefault));
  }
  Region* regs = s->q_regs;
  int* nreg = s->q_nreg;
  for (int bi = 0; bi < nb; ++bi) nreg[bi] = 0;
  int* ovf = s->q_nreg + s->cap_q_box;
  ovf[0] = ovf[1] = 0;
  if (nb > 0) {
    for (int f = 0; f < n_frames; ++f)
      SSLAM_HIP_TRY(hipMemcpyAsync(s->d_cloud + (size_t)f * frame_bytes, frames[f].cloud, frame_bytes, hipMemcpyHostToDevice, s->stream));
    SSLAM_HIP_TRY(hipMemsetAsync(V.overflow, 0, 8 * sizeof(int), s->stream));
    SSLAM_HIP_TRY(hipMemcpyAsync(s->d_box, s->boxes.data(), nb * sizeof(BoxMeta), hipMemcpyHostToDevice, s->stream));
    if (!s->q_e0) { SSLAM_HIP_TRY(hipEventCreate(&s->q_e0)); SSLAM_HIP_TRY(hipEventCreate(&s->q_e1)); }
    hipEvent_t e0 = s->q_e0, e1 = s->q_e1;
    // Two pipelines that start together stay in lock step: both copy at the same time (each at half the PCIe rate), then both run their
    // kernels side by side, and nothing overlaps (rocprofv3 trace of round 5: 2.5 ms of copies without a kernel, then 2.7 ms of kernels
    // without a copy).  The kernels of this batch therefore wait for the peer pipeline's kernels: the copies of batch k + 1 then run under
    // the kernels of batch k by construction, whatever the host's timing.
    if (peer && peer->q_e1 && peer->q_e1_armed) SSLAM_HIP_TRY(hipStreamWaitEvent(s->stream, peer->q_e1, 0));
    SSLAM_HIP_TRY(hipEventRecord(e0, s->stream));
    const dim3 pg((maxpix + 255) / 256, nb), pb(256);
    int maxw = 1;
    for (auto& b : s->boxes) maxw = std::max(maxw, b.w);
    // dynamic LDS: the largest per-box band (the kernels size their bands from the box's own width)
    size_t band_bytes = 0, rband_bytes = 0;
    for (auto& b : s->boxes) {
      const int bh = std::min(64, kBandFloats / b.w - 1);
      band_bytes = std::max(band_bytes, (size_t)(bh + 1) * b.w * sizeof(float));
      const int bhr = std::min(V.refine_bh, kBandFloats / (4 * b.w) - 1);
      rband_bytes = std::max(rband_bytes, (size_t)(bhr + 1) * b.w * 4 * sizeof(float));
    }
    { const int rc_lds = seg_lds_opt_in(s->P.device); if (rc_lds) return rc_lds; }   // > 64 KiB of dynamic LDS for the band / label kernels, once per device
    SSLAM_HIP_TRY(hipMemsetAsync(V.ccount, 0, nb * sizeof(int), s->stream));
    hipLaunchKernelGGL(k_crop, pg, pb, 0, s->stream, V);
    hipLaunchKernelGGL(k_depth_change, pg, pb, 0, s->stream, V);
    hipLaunchKernelGGL(k_distance_map, dim3(nb), dim3(256), band_bytes, s->stream, V);
    {
      // band rows: as many as fit next to the (w+1) x 10 double carry row in ~150 KiB of LDS (<= 64 lanes)
      const size_t carry = (size_t)(maxw + 1) * 10 * sizeof(double);
      // (a call with more boxes than CUs takes 16-row bands: four boxes per CU instead of one)
      const size_t row_cap = nb > 512 ? 16 : 64;   // (1024 boxes of 128 x 96, per call: 12 / 16 / 24 / 32 / 48 / 64 rows 0.599 / 0.551 / 0.604 / 0.606 / 0.680 / 0.706 ms)
      const int ib_rows = (int)std::max<size_t>(1, std::min<size_t>(row_cap, (150 * 1024 - carry) / ((size_t)maxw * 12)));
      const size_t ilds = carry + (size_t)ib_rows * maxw * 12;
      hipLaunchKernelGGL(k_integral, dim3(nb), dim3(256), ilds, s->stream, V, ib_rows);
    }
    hipLaunchKernelGGL(k_normals, pg, pb, 0, s->stream, V);
    if (maxpix <= kCcLdsMax && !getenv("SSLAM_SEG_GLOBAL_CC")) {
      hipLaunchKernelGGL(k_cc_lds, dim3(nb), dim3(1024), (size_t)maxpix * sizeof(int), s->stream, V);
    } else {
      hipLaunchKernelGGL(k_cc_init, pg, pb, 0, s->stream, V);
      hipLaunchKernelGGL(k_cc_merge, pg, pb, 0, s->stream, V);
      hipLaunchKernelGGL(k_cc_flatten, pg, pb, 0, s->stream, V);
      hipLaunchKernelGGL(k_cc_flatten2, pg, pb, 0, s->stream, V);
    }
    if (nb > 256) hipLaunchKernelGGL(k_regions<256>, dim3(nb), dim3(256), 0, s->stream, V);
    else hipLaunchKernelGGL(k_regions<1024>, dim3(nb), dim3(1024), 0, s->stream, V);
    hipLaunchKernelGGL(k_relabel, pg, pb, 0, s->stream, V);
    bool tiles_ok = true;   // k_refine_lds: every thread's tile must fit its 32-bit candidate mask
    for (auto& b : s->boxes) tiles_ok = tiles_ok && ((b.w + kRefTX - 1) / kRefTX) * ((b.h + kRefTY - 1) / kRefTY) <= 32;
    if (maxpix <= kCcLdsMax && tiles_ok && !getenv("SSLAM_SEG_WAVEFRONT_REFINE")) {
      // 16-bit labels + 16-bit masks: 4 bytes per pixel (three 12k-pixel boxes per CU)
      hipLaunchKernelGGL(k_refine_lds, dim3(nb), dim3(kRefTX * kRefTY), (size_t)maxpix * 4 + 8, s->stream, V);
    } else {
      hipLaunchKernelGGL(k_refine, dim3(nb), dim3(256), rband_bytes, s->stream, V);
    }
    size_t cimg_bytes = 0;
    for (auto& b : s->boxes) cimg_bytes = std::max(cimg_bytes, (size_t)(b.w + 2) * (b.h + 2));
    if (cimg_bytes <= 150 * 1024) {
      hipLaunchKernelGGL(k_contour<true>, dim3(nb), dim3(256), cimg_bytes, s->stream, V);
    } else {
      hipLaunchKernelGGL(k_contour<false>, dim3(nb), dim3(256), 0, s->stream, V);
    }
    hipLaunchKernelGGL(k_area, dim3(nb, kMaxRegions), dim3(64), 0, s->stream, V);
    SSLAM_HIP_TRY(hipEventRecord(e1, s->stream));
    s->q_e1_armed = true;
    SSLAM_HIP_TRY(hipMemcpyAsync(regs, V.reg, (size_t)nb * kMaxRegions * sizeof(Region), hipMemcpyDeviceToHost, s->stream));
    SSLAM_HIP_TRY(hipMemcpyAsync(nreg, V.nreg, nb * sizeof(int), hipMemcpyDeviceToHost, s->stream));
    SSLAM_HIP_TRY(hipMemcpyAsync(ovf, V.overflow, 2 * sizeof(int), hipMemcpyDeviceToHost, s->stream));
  }
  s->q_busy = true;
  return 0;
}

// wait for the batch seg_enqueue put on this pipeline, then plane_segmentation.cpp:158-256 + point_cloud_segmentation.h:43-99
// (scalar post-processing)
static int seg_finish(sslam_seg* s, sslam_plane* out, int max_out, int32_t* out_frame) {
  if (!s || (!out && max_out > 0)) return set_error(SSLAM_ERR_INVALID, "null argument");
  if (!s->q_busy) return set_error(SSLAM_ERR_INVALID, "no batch was submitted on this pipeline");
  s->q_busy = false;
  SSLAM_HIP_TRY(hipSetDevice(s->P.device));
  const sslam_seg_params& P = s->P;
  const int nb = (int)s->boxes.size();
  const Region* regs = s->q_regs;
  const int* nreg = s->q_nreg;
  const int* ovf = s->q_nreg + s->cap_q_box;
  float kernel_ms = 0;
  if (nb > 0) {
    SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return set_error(SSLAM_ERR_HIP, "frontend kernels: %s", hipGetErrorString(le));
    SSLAM_HIP_TRY(hipEventElapsedTime(&kernel_ms, s->q_e0, s->q_e1));
  }
  int nout = 0, dropped = 0;
  for (int bi = 0; bi < nb; ++bi) {
    const sslam_seg::FrameMeta& fr = s->q_frames[s->box_frame[bi]];
    const float* robot_pose = fr.robot_pose;
    float T[16];
    sslam_seg_transform(s, robot_pose, fr.cam_angle, T);
    const float hz[3] = {T[8], T[9], T[10]};
    const sslam_seg::BoxInfo& sb = s->q_boxes[bi];
    for (int k = 0; k < nreg[bi]; ++k) {
      const Region& R = regs[(size_t)bi * kMaxRegions + k];
      if (!(R.contour_n > P.min_contour_points)) continue;
      const float* m = R.model;
      const float dotp = hz[0] * m[0] + hz[1] * m[1] + hz[2] * m[2];
      if (!((double)R.area >= P.planar_area)) continue;
      int type = -1;
      float sgn = 1.0f;
      if ((float)(fabsf(m[0]) - fabsf(hz[0])) < 0.3 && (float)(fabsf(m[1]) - fabsf(hz[1])) < 0.3 && (float)(fabsf(m[2]) - fabsf(hz[2])) < 0.3) {
        type = 0;
        if (m[1] > 0) sgn = -1.0f;
      } else if (dotp < 0.5) {
        type = 1;
        if (m[0] > 0) sgn = -1.0f;
      }
      if (type < 0) continue;
      if (nout >= max_out) { ++dropped; continue; }
      if (out_frame) out_frame[nout] = s->box_frame[bi];
      sslam_plane& o = out[nout++];
      memcpy(o.centroid_cam, R.centroid, 12);
      for (int q = 0; q < 4; ++q) o.normal_d[q] = sgn < 0 ? -m[q] : m[q];
      for (int r = 0; r < 3; ++r) {
        float sacc = 0;
        for (int q = 0; q < 3; ++q) sacc += T[r * 4 + q] * R.centroid[q];
        sacc += T[r * 4 + 3] * 1.0f;
        o.world_pose[r] = sacc + robot_pose[r];
      }
      o.num_points = (float)R.contour_n; o.prob = sb.prob; o.plane_type = type; o.class_id = sb.class_id;
      o.box_index = s->box_src[bi]; o.inlier_count = R.inliers; o.area = R.area;
    }
  }
  s->last_dropped_planes = dropped; s->last_candidate_overflow = ovf[0]; s->last_region_overflow = ovf[1];
  s->last_kernel_ms = kernel_ms;
  s->last_total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - s->q_t0).count();
  return nout;
}
static int seg_run(sslam_seg* s, const sslam_frame* frames, int n_frames, int width, int height, int point_step, int row_step, int ox, int oy, int oz,
                   sslam_plane* out, int max_out, int32_t* out_frame) {
  if (!s || !frames || (!out && max_out > 0)) return set_error(SSLAM_ERR_INVALID, "null argument");
  if (s->n_inflight > 0) return set_error(SSLAM_ERR_INVALID, "%d submitted batch(es) must be collected first", s->n_inflight);
  const int rc = seg_enqueue(s, frames, n_frames, width, height, point_step, row_step, ox, oy, oz);
  if (rc) { s->q_busy = false; return rc; }
  return seg_finish(s, out, max_out, out_frame);
}


int sslam_seg_segment(sslam_seg* s, const uint8_t* cloud, int width, int height, int point_step, int row_step, int ox, int oy, int oz,
                      const sslam_box* boxes, int n_boxes, const float robot_pose[6], float cam_angle, sslam_plane* out, int max_out) {
  if (!s || !cloud || (!boxes && n_boxes > 0) || !robot_pose || (!out && max_out > 0)) return set_error(SSLAM_ERR_INVALID, "null argument");
  sslam_frame fr;
  fr.cloud = cloud; fr.boxes = boxes; fr.n_boxes = n_boxes; fr.cam_angle = cam_angle;
  memcpy(fr.robot_pose, robot_pose, sizeof fr.robot_pose);
  return seg_run(s, &fr, 1, width, height, point_step, row_step, ox, oy, oz, out, max_out, nullptr);
}

int sslam_seg_segment_batch(sslam_seg* s, const sslam_frame* frames, int n_frames, int width, int height, int point_step, int row_step,
                            int ox, int oy, int oz, sslam_plane* out, int max_out, int32_t* out_frame) {
  return seg_run(s, frames, n_frames, width, height, point_step, row_step, ox, oy, oz, out, max_out, out_frame);
}

// Pipelined form: at most two batches in flight, on two pipelines (own stream, own device buffers) used in turn; the 9.8 MB-per-frame
// H2D copy of batch k+1 runs under the kernels of batch k.  submit(0); loop { submit(k+1); collect(k); }
int sslam_seg_submit_batch(sslam_seg* s, const sslam_frame* frames, int n_frames, int width, int height, int point_step, int row_step,
                           int ox, int oy, int oz) {
  if (!s) return set_error(SSLAM_ERR_INVALID, "null argument");
  if (s->n_inflight >= 2) return set_error(SSLAM_ERR_INVALID, "two batches are in flight: collect one first");
  int which = 0;
  if (s->n_inflight == 1) which = 1 - s->fifo[0];
  sslam_seg* pipe = s;
  if (which == 1) {
    if (!s->twin) { s->twin = new sslam_seg(); s->twin->P = s->P; }
    pipe = s->twin;
  }
  const int rc = seg_enqueue(pipe, frames, n_frames, width, height, point_step, row_step, ox, oy, oz, pipe == s ? s->twin : s);
  if (rc) { pipe->q_busy = false; return rc; }
  s->fifo[s->n_inflight++] = which;
  return 0;
}
int sslam_seg_collect_batch(sslam_seg* s, sslam_plane* out, int max_out, int32_t* out_frame) {
  if (!s) return set_error(SSLAM_ERR_INVALID, "null argument");
  if (s->n_inflight <= 0) return set_error(SSLAM_ERR_INVALID, "no batch in flight");
  sslam_seg* pipe = s->fifo[0] ? s->twin : s;
  s->fifo[0] = s->fifo[1];
  --s->n_inflight;
  const int n = seg_finish(pipe, out, max_out, out_frame);
  if (pipe != s) {   // the handle reports the last collected batch
    s->last_dropped_planes = pipe->last_dropped_planes; s->last_candidate_overflow = pipe->last_candidate_overflow;
    s->last_region_overflow = pipe->last_region_overflow; s->last_kernel_ms = pipe->last_kernel_ms; s->last_total_ms = pipe->last_total_ms;
  }
  return n;
}

int sslam_seg_last_overflow(const sslam_seg* s, int* dropped_planes, int* boxes_with_full_candidate_table, int* boxes_with_full_region_table) {
  if (!s) return set_error(SSLAM_ERR_INVALID, "null argument");
  if (dropped_planes) *dropped_planes = s->last_dropped_planes;
  if (boxes_with_full_candidate_table) *boxes_with_full_candidate_table = s->last_candidate_overflow;
  if (boxes_with_full_region_table) *boxes_with_full_region_table = s->last_region_overflow;
  return s->last_dropped_planes + s->last_candidate_overflow + s->last_region_overflow;
}

int sslam_seg_ransac_plane(sslam_seg* s, const float* xyz, int n, float threshold, int max_iterations, double probability,
                           uint64_t seed, float coeff_out[4], int32_t* inliers_out, int max_inliers) {
  if (!s || !xyz || !coeff_out || (!inliers_out && max_inliers > 0) || n < 0 || max_iterations < 1)
    return set_error(SSLAM_ERR_INVALID, "bad argument");
  int rc = seg_device(s);
  if (rc) return rc;
  coeff_out[0] = coeff_out[1] = coeff_out[2] = coeff_out[3] = 0;
  if (n < 3) return 0;
  const int H = max_iterations + 1 + max_iterations * 10;   // every hypothesis index the sequential loop can reach (10 skips per iteration)
  float *d_pts = nullptr, *d_models = nullptr;
  int *d_counts = nullptr, *d_blk = nullptr, *d_inl = nullptr, *d_total = nullptr;
  DevGuard g;
  if ((rc = g.alloc(&d_pts, (size_t)n * 3)) || (rc = g.alloc(&d_models, (size_t)(H + 1) * 4)) || (rc = g.alloc(&d_counts, H)) ||
      (rc = g.alloc(&d_blk, (n + 255) / 256)) || (rc = g.alloc(&d_inl, n)) || (rc = g.alloc(&d_total, 1))) return rc;
  SSLAM_HIP_TRY(hipMemcpyAsync(d_pts, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  hipLaunchKernelGGL(k_ransac_score, dim3(H), dim3(256), 0, s->stream, d_pts, n, threshold, (unsigned long long)seed, d_models, d_counts);
  std::vector<int> counts(H);
  SSLAM_HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, (size_t)H * sizeof(int), hipMemcpyDeviceToHost, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  // replay of pcl::RandomSampleConsensus::computeModel over the precomputed counts
  int best = -1, best_it = -1, iterations = 0, skipped = 0;
  double k = 1.0;
  const double log_probability = std::log(1.0 - probability), one_over = 1.0 / (double)n;
  for (int it = 0; it < H && ransac_loop_open(k, iterations, skipped, max_iterations); ++it)
    if (ransac_loop_take(counts[it], one_over, log_probability, k, iterations, skipped, best)) best_it = it;
  if (best <= 0) return 0;
  float* d_model = d_models + (size_t)H * 4;   // working copy of the winning model
  SSLAM_HIP_TRY(hipMemcpyAsync(d_model, d_models + (size_t)best_it * 4, 4 * sizeof(float), hipMemcpyDeviceToDevice, s->stream));
  // inliers of the sampled model -> refit -> inliers of the refined model
  const InlierPred inliers{d_pts, d_model, threshold, d_inl, n};
  int total = 0;
  if ((rc = compact_if(s, inliers, n, d_blk, d_total, nullptr))) return rc;
  hipLaunchKernelGGL(k_ransac_refit, dim3(1), dim3(64), 0, s->stream, d_pts, d_inl, d_total, d_model);
  if ((rc = compact_if(s, inliers, n, d_blk, d_total, &total))) return rc;
  SSLAM_HIP_TRY(hipMemcpy(coeff_out, d_model, 4 * sizeof(float), hipMemcpyDeviceToHost));
  if (total > 0 && max_inliers > 0)
    SSLAM_HIP_TRY(hipMemcpy(inliers_out, d_inl, (size_t)std::min(total, max_inliers) * sizeof(int), hipMemcpyDeviceToHost));
  SSLAM_HIP_TRY(hipGetLastError());
  return total;
}

// ---- RANSAC + ICP over the boxes of the resident batch (configs[3]) ------------------------------------------------------------------
static int seg_resident_check(sslam_seg* s) {
  if (!s) return set_error(SSLAM_ERR_INVALID, "null handle");
  const int rc = seg_have_device();
  if (rc) return rc;
  if (s->q_busy || s->n_inflight > 0) return set_error(SSLAM_ERR_INVALID, "a batch is in flight: collect it first");
  if (!s->stream || s->V.nbox != (int)s->boxes.size()) return set_error(SSLAM_ERR_INVALID, "no resident batch: call sslam_seg_segment / sslam_seg_segment_batch first");
  return 0;
}
static int seg_ransac_lds_opt_in(int device, int* limit) {
  static std::mutex mu;
  static std::vector<std::pair<int, int>> done;
  std::lock_guard<std::mutex> lk(mu);
  for (auto& d : done) if (d.first == device) { *limit = d.second; return 0; }
  const int v = lds_optin_limit(device, 156 * 1024, 4096);
  SSLAM_HIP_TRY(hipFuncSetAttribute((const void*)k_ransac_hyp, hipFuncAttributeMaxDynamicSharedMemorySize, v));
  done.push_back({device, v});
  *limit = v;
  return 0;
}

int sslam_seg_ransac_boxes(sslam_seg* s, float threshold, int max_iterations, double probability, uint64_t seed, sslam_box_plane* out, int max_out,
                           double* kernel_ms) {
  int rc = seg_resident_check(s);
  if (rc) return rc;
  if ((!out && max_out > 0) || max_iterations < 1 || !(threshold > 0) || !(probability > 0 && probability < 1)) return set_error(SSLAM_ERR_INVALID, "bad argument");
  SSLAM_HIP_TRY(hipSetDevice(s->P.device));
  const int nb = (int)s->boxes.size();
  if (kernel_ms) *kernel_ms = 0;
  if (nb == 0) { s->r_nbox = 0; return 0; }
  const size_t npix = (size_t)s->V.npix_total;
  if (npix > s->cap_rflag) {
    if (s->d_rflag) (void)hipFree(s->d_rflag);
    s->d_rflag = nullptr; s->cap_rflag = 0;
    SSLAM_HIP_TRY(hipMalloc((void**)&s->d_rflag, npix));
    s->cap_rflag = npix;
  }
  if ((size_t)nb > s->cap_rbox) {
    if (s->d_rbox) (void)hipFree(s->d_rbox);
    s->d_rbox = nullptr; s->cap_rbox = 0;
    SSLAM_HIP_TRY(hipMalloc(&s->d_rbox, (size_t)nb * sizeof(RansacBox)));
    s->cap_rbox = nb;
  }
  int lds_limit = 0;
  if ((rc = seg_ransac_lds_opt_in(s->P.device, &lds_limit))) return rc;
  // a box whose points fit the LDS is scored out of it; larger boxes read their points through L2
  const int lds_points = std::max(0, (lds_limit - 1024) / 12);
  int max_staged = 0;
  for (auto& b : s->boxes) { const int n = b.w * b.h; if (n <= lds_points) max_staged = std::max(max_staged, n); }
  const size_t lds = (size_t)max_staged * 12 + 16;
  if (!s->q_e0) { SSLAM_HIP_TRY(hipEventCreate(&s->q_e0)); SSLAM_HIP_TRY(hipEventCreate(&s->q_e1)); }
  SSLAM_HIP_TRY(hipEventRecord(s->q_e0, s->stream));
  hipLaunchKernelGGL(k_ransac_hyp, dim3(nb), dim3(1024), lds, s->stream, s->V, threshold, max_iterations, probability, (unsigned long long)seed, lds_points,
                     (RansacBox*)s->d_rbox);
  hipLaunchKernelGGL(k_ransac_refine, dim3(nb), dim3(256), 0, s->stream, s->V, threshold, (RansacBox*)s->d_rbox, s->d_rflag);
  SSLAM_HIP_TRY(hipGetLastError());
  SSLAM_HIP_TRY(hipEventRecord(s->q_e1, s->stream));
  std::vector<RansacBox> rb(nb);
  SSLAM_HIP_TRY(hipMemcpyAsync(rb.data(), s->d_rbox, (size_t)nb * sizeof(RansacBox), hipMemcpyDeviceToHost, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  if (kernel_ms) { float ms = 0; if (hipEventElapsedTime(&ms, s->q_e0, s->q_e1) == hipSuccess) *kernel_ms = ms; }
  s->r_nbox = nb;
  for (int q = 0; q < nb && q < max_out; ++q) {
    sslam_box_plane& o = out[q];
    for (int k = 0; k < 4; ++k) o.coeff[k] = rb[q].coeff[k];
    o.inliers = rb[q].inliers; o.points = s->boxes[q].w * s->boxes[q].h; o.box_index = s->box_src[q]; o.frame = s->box_frame[q];
    o.hypotheses = rb[q].hyps; o.best_iteration = rb[q].best_iter;
  }
  return nb;
}

int sslam_seg_ransac_box_inliers(sslam_seg* s, int slot, int32_t* out, int max_out) {
  int rc = seg_resident_check(s);
  if (rc) return rc;
  if (s->r_nbox < 0) return set_error(SSLAM_ERR_INVALID, "sslam_seg_ransac_boxes has not run on the resident batch");
  if (slot < 0 || slot >= s->r_nbox || (!out && max_out > 0)) return set_error(SSLAM_ERR_INVALID, "bad box slot %d (of %d)", slot, s->r_nbox);
  SSLAM_HIP_TRY(hipSetDevice(s->P.device));
  const BoxMeta& b = s->boxes[slot];
  std::vector<unsigned char> f((size_t)b.w * b.h);
  SSLAM_HIP_TRY(hipMemcpyAsync(f.data(), s->d_rflag + b.pix0, f.size(), hipMemcpyDeviceToHost, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  int n = 0;
  for (size_t i = 0; i < f.size(); ++i) if (f[i]) { if (n < max_out) out[n] = (int32_t)i; ++n; }
  return n;
}

int sslam_seg_icp_boxes(sslam_seg* s, const int32_t* box_plane, int n_boxes, const float* planes, int n_planes, int iterations, const double* T0,
                        sslam_icp_result* out, int max_out, double* kernel_ms) {
  int rc = seg_resident_check(s);
  if (rc) return rc;
  if (s->r_nbox < 0) return set_error(SSLAM_ERR_INVALID, "sslam_seg_ransac_boxes has not run on the resident batch");
  if (!box_plane || !planes || !out || n_boxes != s->r_nbox || n_planes <= 0 || iterations < 0 || max_out < 0) return set_error(SSLAM_ERR_INVALID, "bad argument (the batch holds %d boxes)", s->r_nbox);
  SSLAM_HIP_TRY(hipSetDevice(s->P.device));
  const int nf = (int)s->q_frames.size();
  if (kernel_ms) *kernel_ms = 0;
  if (nf == 0) return 0;
  const int nb = s->r_nbox;
  // one upload: [frame_box0 (nf + 1) | box_frame (nb) | box_plane (nb) | planes (4 n_planes floats) | IcpState (nf)]; scratch lives in the
  // handle and only grows (round-4 ADVICE: five hipMalloc / hipFree pairs per call synchronised the device)
  const size_t o_bf = (size_t)(nf + 1), o_bp = o_bf + nb, o_pl = o_bp + nb;
  const size_t o_st = ((o_pl + (size_t)4 * n_planes) * 4 + 15) / 16 * 16;   // bytes
  const size_t in_bytes = o_st + (size_t)nf * sizeof(IcpState);
  const size_t part_bytes = (size_t)std::max(nb, 1) * kIcpSums * sizeof(double), out_bytes = (size_t)nf * sizeof(IcpFrame);
  const size_t need = (in_bytes + 255) / 256 * 256 + (part_bytes + 255) / 256 * 256 + out_bytes;
  if (s->cap_icp < need) {
    SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->d_icp) (void)hipFree(s->d_icp);
    s->d_icp = nullptr; s->cap_icp = 0;
    SSLAM_HIP_TRY(hipMalloc(&s->d_icp, need + 4096));
    s->cap_icp = need + 4096;
  }
  s->h_icp.assign(in_bytes, 0);
  int* hi = reinterpret_cast<int*>(s->h_icp.data());
  for (int q = 0; q < nb; ++q) hi[s->box_frame[q] + 1]++;   // the slots of a frame are consecutive (frames are packed in order)
  for (int f = 0; f < nf; ++f) hi[f + 1] += hi[f];
  for (int q = 0; q < nb; ++q) { hi[o_bf + q] = s->box_frame[q]; hi[o_bp + q] = box_plane[q]; }
  std::memcpy(hi + o_pl, planes, (size_t)4 * n_planes * sizeof(float));
  IcpState* hs = reinterpret_cast<IcpState*>(s->h_icp.data() + o_st);
  for (int f = 0; f < nf; ++f) {
    for (int k = 0; k < 12; ++k) hs[f].T[k] = T0 ? T0[(size_t)f * 12 + k] : ((k < 9 && k % 4 == 0) ? 1.0 : 0.0);
    hs[f].status = 0; hs[f].done = 0;
  }
  char* base = static_cast<char*>(s->d_icp);
  const int* d_fb0 = reinterpret_cast<const int*>(base);
  const int* d_bf = d_fb0 + o_bf;
  const int* d_bp = d_fb0 + o_bp;
  const float* d_planes = reinterpret_cast<const float*>(d_fb0 + o_pl);
  IcpState* d_st = reinterpret_cast<IcpState*>(base + o_st);
  double* d_part = reinterpret_cast<double*>(base + (in_bytes + 255) / 256 * 256);
  IcpFrame* d_out = reinterpret_cast<IcpFrame*>(reinterpret_cast<char*>(d_part) + (part_bytes + 255) / 256 * 256);
  SSLAM_HIP_TRY(hipMemcpyAsync(base, s->h_icp.data(), in_bytes, hipMemcpyHostToDevice, s->stream));
  if (!s->q_e0) { SSLAM_HIP_TRY(hipEventCreate(&s->q_e0)); SSLAM_HIP_TRY(hipEventCreate(&s->q_e1)); }
  SSLAM_HIP_TRY(hipEventRecord(s->q_e0, s->stream));
  for (int it = 0; it <= iterations; ++it) {
    if (nb > 0) hipLaunchKernelGGL(k_icp_box_sums, dim3(nb), dim3(256), 0, s->stream, s->V, (const unsigned char*)s->d_rflag, d_bf, d_bp, d_planes, n_planes, (const IcpState*)d_st, d_part);
    hipLaunchKernelGGL(k_icp_frame_step, dim3(nf), dim3(64), 0, s->stream, d_fb0, (const double*)d_part, it, iterations, d_st, d_out);
  }
  SSLAM_HIP_TRY(hipGetLastError());
  SSLAM_HIP_TRY(hipEventRecord(s->q_e1, s->stream));
  std::vector<IcpFrame> res(nf);
  SSLAM_HIP_TRY(hipMemcpyAsync(res.data(), d_out, out_bytes, hipMemcpyDeviceToHost, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  if (kernel_ms) { float ms = 0; if (hipEventElapsedTime(&ms, s->q_e0, s->q_e1) == hipSuccess) *kernel_ms = ms; }
  for (int f = 0; f < nf && f < max_out; ++f) {
    for (int k = 0; k < 12; ++k) out[f].T[k] = res[f].T[k];
    out[f].rms = res[f].rms; out[f].used = res[f].used; out[f].status = res[f].status;
  }
  return nf;
}

int sslam_seg_convex_hull_2d(sslam_seg* s, const float* xyz, int n, const int32_t* inliers, int n_inliers, const float coeff[4],
                             float* projected_out, int32_t* hull_out, int max_hull, int* axes_out) {
  if (!s || !xyz || !inliers || !coeff || (!hull_out && max_hull > 0) || n < 0 || n_inliers < 0)
    return set_error(SSLAM_ERR_INVALID, "bad argument");
  int rc = seg_device(s);
  if (rc) return rc;
  if (axes_out) *axes_out = -1;
  if (n_inliers < 3) return set_error(SSLAM_ERR_INVALID, "a 2-D hull needs at least 3 inliers");
  for (int k = 0; k < n_inliers; ++k) if (inliers[k] < 0 || inliers[k] >= n) return set_error(SSLAM_ERR_INVALID, "inlier index out of range");
  const int m0 = n_inliers, nblk = (m0 + 255) / 256;
  const size_t max_chunks = (m0 + kHullCap - 1) / kHullCap;
  float *d_pts = nullptr, *d_proj = nullptr, *d_px = nullptr, *d_py = nullptr, *d_cx = nullptr, *d_cy = nullptr, *d_ox = nullptr, *d_oy = nullptr;
  int *d_inl = nullptr, *d_ci = nullptr, *d_oi = nullptr, *d_meta = nullptr, *d_bidx = nullptr, *d_eidx = nullptr, *d_blk = nullptr, *d_total = nullptr,
      *d_counts = nullptr, *d_off = nullptr;
  double *d_bkey = nullptr, *d_ext = nullptr;
  DevGuard g;
  if ((rc = g.alloc(&d_pts, (size_t)n * 3)) || (rc = g.alloc(&d_inl, m0)) || (rc = g.alloc(&d_proj, (size_t)m0 * 3)) || (rc = g.alloc(&d_px, m0)) ||
      (rc = g.alloc(&d_py, m0)) || (rc = g.alloc(&d_cx, m0)) || (rc = g.alloc(&d_cy, m0)) || (rc = g.alloc(&d_ci, m0)) ||
      (rc = g.alloc(&d_ox, max_chunks * kHullCap)) || (rc = g.alloc(&d_oy, max_chunks * kHullCap)) || (rc = g.alloc(&d_oi, max_chunks * kHullCap)) ||
      (rc = g.alloc(&d_meta, 4)) || (rc = g.alloc(&d_bkey, (size_t)nblk * 8)) || (rc = g.alloc(&d_bidx, (size_t)nblk * 8)) || (rc = g.alloc(&d_ext, 17)) ||
      (rc = g.alloc(&d_eidx, 8)) || (rc = g.alloc(&d_blk, nblk)) || (rc = g.alloc(&d_total, 1)) || (rc = g.alloc(&d_counts, max_chunks)) ||
      (rc = g.alloc(&d_off, max_chunks))) return rc;
  SSLAM_HIP_TRY(hipMemcpyAsync(d_pts, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  SSLAM_HIP_TRY(hipMemcpyAsync(d_inl, inliers, (size_t)m0 * sizeof(int), hipMemcpyHostToDevice, s->stream));
  hipLaunchKernelGGL(k_hull_project, dim3(nblk), dim3(256), 0, s->stream, d_pts, d_inl, m0, coeff[0], coeff[1], coeff[2], coeff[3], d_proj);
  hipLaunchKernelGGL(k_hull_axes, dim3(1), dim3(1), 0, s->stream, d_proj, m0, cosf(0.174532925f), d_meta);
  int axes = -1;
  SSLAM_HIP_TRY(hipMemcpyAsync(&axes, d_meta, sizeof(int), hipMemcpyDeviceToHost, s->stream));
  if (projected_out) SSLAM_HIP_TRY(hipMemcpyAsync(projected_out, d_proj, (size_t)m0 * 3 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  if (axes_out) *axes_out = axes;
  if (axes < 0) return set_error(SSLAM_ERR_NUMERIC, "convex hull: the projected inliers are collinear");
  hipLaunchKernelGGL(k_hull_coords, dim3(nblk), dim3(256), 0, s->stream, d_proj, m0, d_meta, d_px, d_py);
  hipLaunchKernelGGL(k_hull_extreme_partial, dim3(nblk), dim3(256), 0, s->stream, d_px, d_py, m0, d_bkey, d_bidx);
  hipLaunchKernelGGL(k_hull_extreme_final, dim3(1), dim3(64), 0, s->stream, d_bkey, d_bidx, nblk, d_px, d_py, d_ext, d_eidx);
  int m = 0;
  if ((rc = compact_if(s, HullPred{d_px, d_py, d_ext, d_cx, d_cy, d_ci}, m0, d_blk, d_total, &m))) return rc;
  while (m > kHullCap) {   // hull of hulls until one workgroup holds every candidate
    const int nchunks = (m + kHullCap - 1) / kHullCap;
    hipLaunchKernelGGL(k_hull_core<false>, dim3(nchunks), dim3(1024), 0, s->stream, d_cx, d_cy, d_ci, m, d_ox, d_oy, d_oi, d_counts);
    hipLaunchKernelGGL(k_exclusive_scan, dim3(1), dim3(64), 0, s->stream, d_counts, nchunks, d_off, d_total);
    hipLaunchKernelGGL(k_hull_compact, dim3(nchunks), dim3(256), 0, s->stream, d_ox, d_oy, d_oi, d_counts, d_off, d_cx, d_cy, d_ci);
    int m2 = 0;
    SSLAM_HIP_TRY(hipMemcpyAsync(&m2, d_total, sizeof(int), hipMemcpyDeviceToHost, s->stream));
    SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
    if (m2 >= m) return set_error(SSLAM_ERR_UNSUPPORTED, "convex hull with more than %d vertices", kHullCap);
    m = m2;
  }
  hipLaunchKernelGGL(k_hull_core<true>, dim3(1), dim3(1024), 0, s->stream, d_cx, d_cy, d_ci, m, d_ox, d_oy, d_oi, d_counts);
  int h = 0;
  SSLAM_HIP_TRY(hipMemcpyAsync(&h, d_counts, sizeof(int), hipMemcpyDeviceToHost, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  if (h > 0 && max_hull > 0) SSLAM_HIP_TRY(hipMemcpy(hull_out, d_oi, (size_t)std::min(h, max_hull) * sizeof(int), hipMemcpyDeviceToHost));
  SSLAM_HIP_TRY(hipGetLastError());
  return h;
}

static int seg_find_slot(sslam_seg* s, int box) {
  for (size_t k = 0; k < s->box_src.size(); ++k) if (s->box_src[k] == box && s->box_frame[k] == 0) return (int)k;   // parity hooks address frame 0
  return -1;
}
int sslam_seg_get_normals(sslam_seg* s, int box, float* out) {
  if (!s || !out) return set_error(SSLAM_ERR_INVALID, "null argument");
  const int k = seg_find_slot(s, box);
  if (k < 0) return set_error(SSLAM_ERR_INVALID, "box %d was rejected or skipped in the last call", box);
  const BoxMeta& b = s->boxes[k];
  SSLAM_HIP_TRY(hipMemcpy(out, s->V.nrm + (size_t)b.pix0 * 4, (size_t)b.w * b.h * 4 * sizeof(float), hipMemcpyDeviceToHost));
  return b.w * b.h;
}
int sslam_seg_get_labels(sslam_seg* s, int box, int32_t* out) {
  if (!s || !out) return set_error(SSLAM_ERR_INVALID, "null argument");
  const int k = seg_find_slot(s, box);
  if (k < 0) return set_error(SSLAM_ERR_INVALID, "box %d was rejected or skipped in the last call", box);
  const BoxMeta& b = s->boxes[k];
  const int n = b.w * b.h;
  int* d = nullptr;
  SSLAM_HIP_TRY(hipMalloc((void**)&d, (size_t)n * sizeof(int)));
  hipLaunchKernelGGL(k_label_image, dim3((n + 255) / 256), dim3(256), 0, s->stream, s->V, k, d);
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  SSLAM_HIP_TRY(hipMemcpy(out, d, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  (void)hipFree(d);
  return n;
}
int sslam_seg_last_timing(const sslam_seg* s, double* kernel_ms, double* total_ms) {
  if (!s) return set_error(SSLAM_ERR_INVALID, "null argument");
  if (kernel_ms) *kernel_ms = s->last_kernel_ms;
  if (total_ms) *total_ms = s->last_total_ms;
  return 0;
}


// Point-to-plane ICP of labelled points against a set of planes (see k_icp_accumulate).  T_out = R (row-major) | t, 12 doubles.
int sslam_seg_icp_point_to_plane(sslam_seg* s, const float* xyz, const int32_t* labels, int n, const float* planes, int n_planes,
                                 int iterations, const double T0[12], double T_out[12], double* rms_out) {
  if (!s || !xyz || !labels || !planes || !T_out || n < 0 || n_planes <= 0 || iterations < 0) return set_error(SSLAM_ERR_INVALID, "bad argument");
  int rc = seg_device(s);
  if (rc) return rc;
  IcpPose T;
  for (int k = 0; k < 12; ++k) T.T[k] = T0 ? T0[k] : ((k < 9 && k % 4 == 0) ? 1.0 : 0.0);
  const int nblk = std::max(1, std::min(256, (n + 255) / 256));
  float *d_pts = nullptr, *d_planes = nullptr;
  int* d_lab = nullptr;
  double* d_part = nullptr;
  DevGuard g;
  if ((rc = g.alloc(&d_pts, (size_t)n * 3)) || (rc = g.alloc(&d_lab, n)) || (rc = g.alloc(&d_planes, (size_t)n_planes * 4)) ||
      (rc = g.alloc(&d_part, (size_t)nblk * kIcpSums))) return rc;
  if (n > 0) {
    SSLAM_HIP_TRY(hipMemcpyAsync(d_pts, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s->stream));
    SSLAM_HIP_TRY(hipMemcpyAsync(d_lab, labels, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s->stream));
  }
  SSLAM_HIP_TRY(hipMemcpyAsync(d_planes, planes, (size_t)n_planes * 4 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  std::vector<double> part((size_t)nblk * kIcpSums);
  double sums[kIcpSums];
  auto accumulate = [&]() -> int {
    hipLaunchKernelGGL(k_icp_accumulate, dim3(nblk), dim3(256), 0, s->stream, d_pts, d_lab, n, d_planes, n_planes, T, d_part);
    SSLAM_HIP_TRY(hipGetLastError());
    SSLAM_HIP_TRY(hipMemcpyAsync(part.data(), d_part, part.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
    for (int k = 0; k < kIcpSums; ++k) { double v = 0; for (int b = 0; b < nblk; ++b) v += part[(size_t)b * kIcpSums + k]; sums[k] = v; }
    return 0;
  };
  for (int it = 0; it < iterations; ++it) {
    if ((rc = accumulate())) return rc;
    if (sums[28] < 6) break;
    if (!icp_gn_step(sums, T.T))
      return set_error(SSLAM_ERR_NUMERIC, "point-to-plane system is rank deficient (the planes do not constrain all six degrees of freedom)");
  }
  if ((rc = accumulate())) return rc;   // residual at the returned transform
  for (int k = 0; k < 12; ++k) T_out[k] = T.T[k];
  if (rms_out) *rms_out = sums[28] > 0 ? std::sqrt(sums[27] / sums[28]) : 0.0;
  return (int)sums[28];
}


// ---- cloud filters ------------------------------------------------------------------------------------------------

int sslam_seg_distance_filter(sslam_seg* s, const float* xyz, int n, double dmin, double dmax, int32_t* keep_out, int max_out) {
  if (!s || !xyz || n < 0 || (!keep_out && max_out > 0)) return set_error(SSLAM_ERR_INVALID, "bad argument");
  int rc = seg_device(s);
  if (rc) return rc;
  if (n == 0) return 0;
  DevGuard g;
  float* d_pts = nullptr; unsigned char* d_flag = nullptr; int* d_out = nullptr;
  if ((rc = g.alloc(&d_pts, (size_t)n * 3)) || (rc = g.alloc(&d_flag, n)) || (rc = g.alloc(&d_out, n))) return rc;
  SSLAM_HIP_TRY(hipMemcpyAsync(d_pts, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  hipLaunchKernelGGL(k_range_flag, dim3((n + 255) / 256), dim3(256), 0, s->stream, d_pts, n, dmin, dmax, d_flag);
  int total = 0;
  if ((rc = compact_flags(s, g, d_flag, n, d_out, n, &total))) return rc;
  const int m = std::min(total, max_out);
  if (m > 0) SSLAM_HIP_TRY(hipMemcpy(keep_out, d_out, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
  return total;
}

// pcl::VoxelGrid::applyFilter: inverse leaf size, integer bounds of the box of the finite points, cells per axis.  Host only, and the
// one copy of the rule: the cell of a point is (int)floorf(x * inv) - minb on the device, which stays inside [0, div) exactly when both
// bounds are representable, so every bound is compared as a float BEFORE its cast (a cast out of range is undefined on the host and
// saturates on the device), and the cell count is bounded before anything is sized by it.
// With shift > 0 the grid is one of BRICKS of 2^shift cells per axis (the map cloud, shift 3): the cell bounds pass the same 32-bit test,
// minb and div are in bricks (cell >> shift, an arithmetic shift), and the bound of 2^26 is on the bricks.
static int voxel_geometry(const float lo[3], const float hi[3], float leaf, VoxelGeom* G, long long div[3], long long* ncell_out, int shift = 0) {
  if (!(leaf > 0)) return set_error(SSLAM_ERR_INVALID, "bad argument (leaf must be positive)");
  const float inv = 1.0f / leaf;
  if (!std::isfinite(inv)) return set_error(SSLAM_ERR_UNSUPPORTED, "voxel grid: 1 / leaf is not finite (leaf %g)", (double)leaf);
  const long long max_cells = 1ll << 26;
  long long ncell = 1;
  bool too_many = false;
  for (int k = 0; k < 3; ++k) {
    const float fl = std::floor(lo[k] * inv), fh = std::floor(hi[k] * inv);
    if (!(fl >= -2147483648.0f && fl < 2147483648.0f && fh >= -2147483648.0f && fh < 2147483648.0f))
      return set_error(SSLAM_ERR_UNSUPPORTED, "voxel grid: the cell index of a bound (%g .. %g at leaf %g) does not fit 32 bits", (double)lo[k], (double)hi[k], (double)leaf);
    G->inv[k] = inv;
    G->minb[k] = (int)fl >> shift;
    div[k] = (long long)((int)fh >> shift) - G->minb[k] + 1;
    if (div[k] < 1) return set_error(SSLAM_ERR_UNSUPPORTED, "voxel grid: upper bound below the lower bound on axis %d", k);
  }
  for (int k = 0; k < 3; ++k) {
    if (div[k] > max_cells / ncell) too_many = true; else ncell *= div[k];
  }
  if (too_many)
    return set_error(SSLAM_ERR_UNSUPPORTED, "voxel grid of %.0f %s: leaf size too small for the extent of the cloud (PCL refuses as well)",
                     (double)div[0] * (double)div[1] * (double)div[2], shift ? "bricks" : "cells");
  *ncell_out = ncell;
  return 0;
}
int sslam_debug_voxel_geometry(const float lo[3], const float hi[3], float leaf, int32_t minb[3], int64_t div[3]) {
  if (!lo || !hi || !minb || !div) return set_error(SSLAM_ERR_INVALID, "bad argument");
  VoxelGeom G;
  long long d[3], ncell = 0;
  const int rc = voxel_geometry(lo, hi, leaf, &G, d, &ncell);
  if (rc) return rc;
  for (int k = 0; k < 3; ++k) { minb[k] = G.minb[k]; div[k] = d[k]; }
  return 0;
}

// the voxel grid over n > 0 points that sit on the device: min / max, geometry, accumulate, the ascending list of the occupied cells, the
// centroids.  *d_out (3 floats per voxel) and *d_oc (points per voxel) are the guard's and stay NULL with *nocc = 0 (no finite point).
// The host reads back the bounding box and the number of occupied cells; everything else stays on the device.
static int voxel_grid_device(sslam_seg* s, DevGuard& g, const float* d_pts, int n, float leaf, float** d_out, int** d_oc, int* nocc_out) {
  int rc;
  *d_out = nullptr; *d_oc = nullptr; *nocc_out = 0;
  float* d_part = nullptr;
  const int nblk = std::min(256, (n + 255) / 256);
  if ((rc = g.alloc(&d_part, (size_t)nblk * 6))) return rc;
  hipLaunchKernelGGL(k_voxel_minmax, dim3(nblk), dim3(256), 0, s->stream, d_pts, n, d_part);
  std::vector<float> part((size_t)nblk * 6);
  SSLAM_HIP_TRY(hipMemcpyAsync(part.data(), d_part, part.size() * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  float lo[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f}, hi[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
  for (int b = 0; b < nblk; ++b) for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], part[(size_t)b * 6 + k]); hi[k] = std::max(hi[k], part[(size_t)b * 6 + 3 + k]); }
  if (!(lo[0] <= hi[0])) return 0;   // no finite point
  VoxelGeom G;
  long long div[3], ncell = 0;
  if ((rc = voxel_geometry(lo, hi, leaf, &G, div, &ncell))) return rc;
  G.mul[0] = 1; G.mul[1] = (int)div[0]; G.mul[2] = (int)(div[0] * div[1]);
  int* d_count = nullptr; long long* d_sums = nullptr; unsigned char* d_flag = nullptr; int* d_cells = nullptr;
  if ((rc = g.alloc(&d_count, (size_t)ncell)) || (rc = g.alloc(&d_sums, (size_t)ncell * 3)) || (rc = g.alloc(&d_flag, (size_t)ncell)) || (rc = g.alloc(&d_cells, (size_t)ncell))) return rc;
  SSLAM_HIP_TRY(hipMemsetAsync(d_count, 0, (size_t)ncell * sizeof(int), s->stream));
  SSLAM_HIP_TRY(hipMemsetAsync(d_sums, 0, (size_t)ncell * 3 * sizeof(long long), s->stream));
  hipLaunchKernelGGL(k_voxel_accumulate, dim3((n + 255) / 256), dim3(256), 0, s->stream, d_pts, n, G, d_count, d_sums);
  hipLaunchKernelGGL(k_voxel_flag, dim3((int)((ncell + 255) / 256)), dim3(256), 0, s->stream, d_count, (int)ncell, d_flag);
  int nocc = 0;
  if ((rc = compact_flags(s, g, d_flag, (int)ncell, d_cells, (int)ncell, &nocc))) return rc;
  if (nocc == 0) return 0;
  if ((rc = g.alloc(d_out, (size_t)nocc * 3)) || (rc = g.alloc(d_oc, nocc))) return rc;
  hipLaunchKernelGGL(k_voxel_centroids, dim3((nocc + 255) / 256), dim3(256), 0, s->stream, d_cells, nocc, d_count, d_sums, *d_out, *d_oc);
  SSLAM_HIP_TRY(hipGetLastError());
  *nocc_out = nocc;
  return 0;
}
int sslam_seg_voxel_grid(sslam_seg* s, const float* xyz, int n, float leaf, float* centroids_out, int32_t* counts_out, int max_out) {
  if (!s || !xyz || n < 0 || !(leaf > 0) || (!centroids_out && max_out > 0)) return set_error(SSLAM_ERR_INVALID, "bad argument");
  int rc = seg_device(s);
  if (rc) return rc;
  if (n == 0) return 0;
  DevGuard g;
  float *d_pts = nullptr, *d_out = nullptr;
  int* d_oc = nullptr;
  if ((rc = g.alloc(&d_pts, (size_t)n * 3))) return rc;
  SSLAM_HIP_TRY(hipMemcpyAsync(d_pts, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  int nocc = 0;
  if ((rc = voxel_grid_device(s, g, d_pts, n, leaf, &d_out, &d_oc, &nocc))) return rc;
  if (nocc == 0) return 0;
  const int m = std::min(nocc, max_out);
  if (m > 0) {
    SSLAM_HIP_TRY(hipMemcpyAsync(centroids_out, d_out, (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    if (counts_out) SSLAM_HIP_TRY(hipMemcpyAsync(counts_out, d_oc, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, s->stream));
  }
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  return nocc;
}

// ---- map cloud (the contract is at sslam_seg_map_cloud in include/sslam.h) -------------------------------------------------------------
}  // extern "C"
namespace sslam {
int seg_map_cloud_device(sslam_seg* s, const MapCloudIn& in, float resolution, int min_points, float* xyz_out, int32_t* cells_out, int32_t* counts_out,
                         int max_out, sslam_map_stats* stats) {
  if (!s || in.n_clouds < 0) return set_error(SSLAM_ERR_INVALID, "bad argument");
  int rc = map_cloud_check_args(resolution, min_points, xyz_out, max_out);
  if (rc) return rc;
  if (s->q_busy || s->n_inflight > 0) return set_error(SSLAM_ERR_INVALID, "a batch is in flight: collect it first");
  if (in.n_clouds > (1 << 22)) return set_error(SSLAM_ERR_UNSUPPORTED, "map cloud: %d clouds, more than 2^22 (one launch row per cloud)", in.n_clouds);
  if ((rc = seg_device(s))) return rc;
  sslam_map_stats st;
  std::memset(&st, 0, sizeof st);
  const int nc = in.n_clouds;
  st.n_clouds = nc;
  int max_len = 0;
  if (nc > 0) {
    st.n_points = in.h_start[nc] - in.h_start[0];
    for (int c = 0; c < nc; ++c) max_len = std::max(max_len, in.h_start[c + 1] - in.h_start[c]);
  }
  for (double& v : s->map_pass_ms) v = 0;
  if (stats) *stats = st;
  if (max_len == 0) return 0;
  for (hipEvent_t& e : s->m_ev) if (!e) SSLAM_HIP_TRY(hipEventCreate(&e));
  const MapIn M{in.d_xyz, in.d_start, in.d_pose};
  const dim3 grid((unsigned)nc, (unsigned)std::min((max_len + 255) / 256, 8192)), block(256);
  DevGuard g;
  // pass 0: the box of the transformed points
  int* d_box = nullptr;
  if ((rc = g.alloc(&d_box, 8))) return rc;
  int h_box[8] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN, 0, 0};   // [6]: points used; [7]: voxels occupied before min_points
  SSLAM_HIP_TRY(hipMemcpyAsync(d_box, h_box, sizeof h_box, hipMemcpyHostToDevice, s->stream));
  SSLAM_HIP_TRY(hipEventRecord(s->m_ev[0], s->stream));
  const dim3 grid_box((unsigned)nc, std::min(grid.y, (unsigned)std::max(1, 2048 / nc)));
  hipLaunchKernelGGL(k_map_minmax, grid_box, block, 0, s->stream, M, d_box);
  SSLAM_HIP_TRY(hipGetLastError());
  SSLAM_HIP_TRY(hipEventRecord(s->m_ev[1], s->stream));
  SSLAM_HIP_TRY(hipMemcpyAsync(h_box, d_box, 6 * sizeof(int), hipMemcpyDeviceToHost, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  auto pass_ms = [&](int k) -> int {
    float ms = 0.0f;
    SSLAM_HIP_TRY(hipEventElapsedTime(&ms, s->m_ev[2 * k], s->m_ev[2 * k + 1]));
    s->map_pass_ms[k] = (double)ms;
    st.kernel_ms += (double)ms;
    return 0;
  };
  if ((rc = pass_ms(0))) return rc;
  if (stats) *stats = st;
  if (h_box[0] > h_box[3]) return 0;   // no usable point
  float lo[3], hi[3];
  for (int k = 0; k < 3; ++k) {        // map_ordered is its own inverse
    const int a = h_box[k] ^ ((h_box[k] >> 31) & 0x7fffffff), b = h_box[3 + k] ^ ((h_box[3 + k] >> 31) & 0x7fffffff);
    std::memcpy(&lo[k], &a, 4); std::memcpy(&hi[k], &b, 4);
  }
  VoxelGeom G;
  long long div[3], nbrick = 0;
  if ((rc = voxel_geometry(lo, hi, resolution, &G, div, &nbrick, 3))) return rc;
  G.mul[0] = 1; G.mul[1] = (int)div[0]; G.mul[2] = (int)(div[0] * div[1]);
  // pass 1: the occupied bricks, their ascending list and the brick -> slot table
  unsigned char* d_flag = nullptr; int *d_list = nullptr, *d_slot = nullptr, *d_blk = nullptr, *d_total = nullptr;
  if ((rc = g.alloc(&d_flag, (size_t)nbrick)) || (rc = g.alloc(&d_list, (size_t)std::min<long long>(nbrick, st.n_points))) || (rc = g.alloc(&d_slot, (size_t)nbrick)) ||
      (rc = g.alloc(&d_blk, (size_t)((nbrick + 255) / 256))) || (rc = g.alloc(&d_total, 1))) return rc;
  SSLAM_HIP_TRY(hipMemsetAsync(d_flag, 0, (size_t)nbrick, s->stream));
  SSLAM_HIP_TRY(hipEventRecord(s->m_ev[2], s->stream));
  hipLaunchKernelGGL(k_map_flag_bricks, grid, block, 0, s->stream, M, G, d_flag);
  int nocc = 0;
  if ((rc = compact_if(s, BrickPred{d_flag, d_list, d_slot}, (int)nbrick, d_blk, d_total, nullptr, true))) return rc;
  SSLAM_HIP_TRY(hipEventRecord(s->m_ev[3], s->stream));
  SSLAM_HIP_TRY(hipMemcpyAsync(&nocc, d_total, sizeof(int), hipMemcpyDeviceToHost, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  if ((rc = pass_ms(1))) return rc;
  if (nocc > (1 << 20))
    return set_error(SSLAM_ERR_UNSUPPORTED, "map cloud: %d occupied bricks of 8 x 8 x 8 cells, more than 2^20: resolution %g is too fine for these clouds", nocc, (double)resolution);
  st.n_bricks = nocc;
  // pass 2: count and fixed-point sums of every voxel of the occupied bricks
  const size_t nvox = (size_t)nocc * 512;
  int* d_count = nullptr; long long* d_sums = nullptr;
  if ((rc = g.alloc(&d_count, nvox)) || (rc = g.alloc(&d_sums, nvox * 3))) return rc;
  SSLAM_HIP_TRY(hipMemsetAsync(d_count, 0, nvox * sizeof(int), s->stream));
  SSLAM_HIP_TRY(hipMemsetAsync(d_sums, 0, nvox * 3 * sizeof(long long), s->stream));
  SSLAM_HIP_TRY(hipEventRecord(s->m_ev[4], s->stream));
  hipLaunchKernelGGL(k_map_accumulate, grid, block, 0, s->stream, M, G, d_slot, d_count, d_sums, d_box + 6);
  SSLAM_HIP_TRY(hipGetLastError());
  SSLAM_HIP_TRY(hipEventRecord(s->m_ev[5], s->stream));
  // pass 3: the voxels that pass min_points, in ascending slot * 512 + local, and their records
  const int thr = std::max(min_points, 1);
  const int cap_list = (int)std::min<size_t>(nvox, (size_t)std::min(max_out, st.n_points));
  int *d_vox = nullptr, *d_vblk = nullptr;
  if ((rc = g.alloc(&d_vox, (size_t)cap_list)) || (rc = g.alloc(&d_vblk, (nvox + 255) / 256))) return rc;
  SSLAM_HIP_TRY(hipEventRecord(s->m_ev[6], s->stream));
  int total = 0;
  if (thr > 1) {   // n_voxels counts before min_points; it is read with n_used at the end
    hipLaunchKernelGGL(k_count_if<VoxelPred>, dim3((unsigned)((nvox + 255) / 256)), dim3(256), 0, s->stream, VoxelPred{d_count, 1, nullptr, 0}, (int)nvox, d_vblk);
    hipLaunchKernelGGL(k_exclusive_scan_wide, dim3(1), dim3(1024), 0, s->stream, d_vblk, (int)((nvox + 255) / 256), d_vblk, d_box + 7);
  }
  if ((rc = compact_if(s, VoxelPred{d_count, thr, d_vox, cap_list}, (int)nvox, d_vblk, d_total, &total, true))) return rc;
  const int m = std::min(total, cap_list);
  float* d_out = nullptr; int *d_cell = nullptr, *d_oc = nullptr;
  if (m > 0) {
    if ((rc = g.alloc(&d_out, (size_t)m * 3)) || (rc = g.alloc(&d_cell, (size_t)m * 3)) || (rc = g.alloc(&d_oc, (size_t)m))) return rc;
    hipLaunchKernelGGL(k_map_emit, dim3((m + 255) / 256), dim3(256), 0, s->stream, d_vox, m, d_list, G, (int)div[0], (int)div[1], d_count, d_sums, d_out, d_cell, d_oc);
    SSLAM_HIP_TRY(hipGetLastError());
  }
  SSLAM_HIP_TRY(hipEventRecord(s->m_ev[7], s->stream));
  int tail[2] = {0, 0};   // n_used, n_voxels: waited for below, and on an error return by the guard's hipFree before this frame ends
  SSLAM_HIP_TRY(hipMemcpyAsync(tail, d_box + 6, sizeof tail, hipMemcpyDeviceToHost, s->stream));
  if (m > 0) {
    SSLAM_HIP_TRY(hipMemcpyAsync(xyz_out, d_out, (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    if (cells_out) SSLAM_HIP_TRY(hipMemcpyAsync(cells_out, d_cell, (size_t)m * 3 * sizeof(int), hipMemcpyDeviceToHost, s->stream));
    if (counts_out) SSLAM_HIP_TRY(hipMemcpyAsync(counts_out, d_oc, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, s->stream));
  }
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  if ((rc = pass_ms(2)) || (rc = pass_ms(3))) return rc;
  st.n_used = tail[0];
  st.n_voxels = thr > 1 ? tail[1] : total;
  if (stats) *stats = st;
  return total;
}
int seg_device_index(const sslam_seg* s) { return s->P.device; }
}  // namespace sslam
extern "C" {

// the cloud arguments shared by sslam_seg_map_cloud and sslam_seg_occupancy_map: their checks (n_points: the rows of xyz that are read) ...
static int map_check_clouds(const char* what, const float* xyz, const int32_t* cloud_start, int n_clouds, const double* T, int* n_points) {
  *n_points = 0;
  if (n_clouds < 0 || (n_clouds > 0 && (!cloud_start || !T))) return set_error(SSLAM_ERR_INVALID, "bad argument");
  if (n_clouds == 0) return 0;
  if (cloud_start[0] < 0) return set_error(SSLAM_ERR_INVALID, "cloud_start[0] is negative");
  for (int c = 0; c < n_clouds; ++c)
    if (cloud_start[c + 1] < cloud_start[c]) return set_error(SSLAM_ERR_INVALID, "cloud_start decreases at cloud %d", c);
  *n_points = cloud_start[n_clouds];   // rows of xyz that are read; those below cloud_start[0] belong to no cloud
  if (*n_points > 0 && !xyz) return set_error(SSLAM_ERR_INVALID, "null xyz");
  for (size_t k = 0; k < 12 * (size_t)n_clouds; ++k)
    if (!std::isfinite(T[k])) return set_error(SSLAM_ERR_INVALID, "%s: entry %d of the pose of cloud %d is not finite", what, (int)(k % 12), (int)(k / 12));
  return 0;
}
// ... and their way to the device (the poses cast to float once); *bytes: what travelled
static int map_stage_clouds(sslam_seg* s, DevGuard& g, const float* xyz, const int32_t* cloud_start, int n_clouds, const double* T, int n_points,
                            MapCloudIn* in, int64_t* bytes) {
  int rc;
  float *d_xyz = nullptr, *d_pose = nullptr; int* d_start = nullptr;
  if ((rc = g.alloc(&d_xyz, (size_t)n_points * 3)) || (rc = g.alloc(&d_pose, (size_t)n_clouds * 12)) || (rc = g.alloc(&d_start, (size_t)n_clouds + 1))) return rc;
  std::vector<float> pose(12 * (size_t)n_clouds);
  for (size_t k = 0; k < pose.size(); ++k) pose[k] = (float)T[k];
  const size_t b[3] = {(size_t)n_points * 3 * sizeof(float), pose.size() * sizeof(float), ((size_t)n_clouds + 1) * sizeof(int32_t)};
  SSLAM_HIP_TRY(hipMemcpyAsync(d_xyz, xyz, b[0], hipMemcpyHostToDevice, s->stream));
  SSLAM_HIP_TRY(hipMemcpyAsync(d_pose, pose.data(), b[1], hipMemcpyHostToDevice, s->stream));
  SSLAM_HIP_TRY(hipMemcpyAsync(d_start, cloud_start, b[2], hipMemcpyHostToDevice, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  in->d_xyz = d_xyz; in->d_start = d_start; in->d_pose = d_pose;
  *bytes = (int64_t)(b[0] + b[1] + b[2]);
  return 0;
}

int sslam_seg_map_cloud(sslam_seg* s, const float* xyz, const int32_t* cloud_start, int n_clouds, const double* T, float resolution, int min_points,
                        float* xyz_out, int32_t* cells_out, int32_t* counts_out, int max_out, sslam_map_stats* stats) {
  if (!s) return set_error(SSLAM_ERR_INVALID, "bad argument");
  int n_points = 0, rc;
  if ((rc = map_check_clouds("map cloud", xyz, cloud_start, n_clouds, T, &n_points))) return rc;
  MapCloudIn in{nullptr, nullptr, nullptr, cloud_start, n_clouds};
  if (n_points == 0) return seg_map_cloud_device(s, in, resolution, min_points, xyz_out, cells_out, counts_out, max_out, stats);   // the checks, then 0
  // the argument checks of the device entry come before anything is staged
  if ((rc = map_cloud_check_args(resolution, min_points, xyz_out, max_out))) return rc;
  if (s->q_busy || s->n_inflight > 0) return set_error(SSLAM_ERR_INVALID, "a batch is in flight: collect it first");
  if ((rc = seg_device(s))) return rc;
  DevGuard g;
  int64_t bytes = 0;
  if ((rc = map_stage_clouds(s, g, xyz, cloud_start, n_clouds, T, n_points, &in, &bytes))) return rc;
  rc = seg_map_cloud_device(s, in, resolution, min_points, xyz_out, cells_out, counts_out, max_out, stats);
  if (stats) stats->upload_bytes = bytes;
  return rc;
}

int sslam_seg_last_map_timing(const sslam_seg* s, double ms[4]) {
  if (!s || !ms) return set_error(SSLAM_ERR_INVALID, "null argument");
  for (int k = 0; k < 4; ++k) ms[k] = s->map_pass_ms[k];
  return 0;
}

// ---- occupancy map (the contract is at sslam_seg_occupancy_map in include/sslam.h) --------------------------------------------------------
}  // extern "C"
namespace {
// what the checks and passes 0 and 1 leave for the passes that follow, shared by the ray entry and the scan entry
struct OccFront {
  MapIn M; OccDev P; OccLog L; dim3 grid; VoxelGeom G; long long div[3];
  int* d_box;                      // [0..5] box, [6..9] rays, truncated, outside z, too far, [10] known cells before emit, [12..13] n_steps (one 64-bit word), [14..15] free
  int *d_list, *d_slot, *d_total;  // the touched bricks ascending, brick -> slot, the compactions' counter
  int nocc;                        // touched bricks
  sslam_occ_stats st;
};
int occ_pass_ms(sslam_seg* s, sslam_occ_stats& st, int k) {
  float ms = 0.0f;
  SSLAM_HIP_TRY(hipEventElapsedTime(&ms, s->m_ev[2 * k], s->m_ev[2 * k + 1]));
  s->occ_pass_ms[k] = (double)ms;
  st.kernel_ms += (double)ms;
  return 0;
}
// Returns 1 when passes 2 and 3 are to follow, 0 when the call ends here with no record (*stats is filled), an error otherwise.
int occ_front(sslam_seg* s, const MapCloudIn& in, const sslam_occ_params* p, int max_out, sslam_occ_stats* stats, DevGuard& g, OccFront& F) {
  if (!s || in.n_clouds < 0) return set_error(SSLAM_ERR_INVALID, "bad argument");
  int rc = occupancy_check_args(p, max_out);
  if (rc) return rc;
  if (s->q_busy || s->n_inflight > 0) return set_error(SSLAM_ERR_INVALID, "a batch is in flight: collect it first");
  if (in.n_clouds > (1 << 22)) return set_error(SSLAM_ERR_UNSUPPORTED, "occupancy map: %d clouds, more than 2^22 (one launch row per cloud)", in.n_clouds);
  if ((rc = seg_device(s))) return rc;
  sslam_occ_stats& st = F.st;
  std::memset(&st, 0, sizeof st);
  const int nc = in.n_clouds;
  st.n_clouds = nc;
  int max_len = 0;
  if (nc > 0) {
    st.n_points = in.h_start[nc] - in.h_start[0];
    for (int c = 0; c < nc; ++c) max_len = std::max(max_len, in.h_start[c + 1] - in.h_start[c]);
  }
  for (double& v : s->occ_pass_ms) v = 0;
  if (stats) *stats = st;
  if (max_len == 0) return 0;
  for (hipEvent_t& e : s->m_ev) if (!e) SSLAM_HIP_TRY(hipEventCreate(&e));
  const MapIn M = F.M = MapIn{in.d_xyz, in.d_start, in.d_pose};
  const OccDev P = F.P = OccDev{1.0f / p->resolution, p->z_min, p->z_max, {p->sensor_origin[0], p->sensor_origin[1], p->sensor_origin[2]}, (int)occupancy_range_units(*p)};
  F.L = OccLog{p->l_hit, p->l_miss, p->l_min, p->l_max, p->l_occ};
  const dim3 grid = F.grid = dim3((unsigned)nc, (unsigned)std::min((max_len + 255) / 256, 8192)), block(256);
  // pass 0: the box of the start and end cells, and the ray counters
  int*& d_box = F.d_box;
  if ((rc = g.alloc(&d_box, 16))) return rc;
  int h_box[16] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN};
  SSLAM_HIP_TRY(hipMemcpyAsync(d_box, h_box, sizeof h_box, hipMemcpyHostToDevice, s->stream));
  SSLAM_HIP_TRY(hipEventRecord(s->m_ev[0], s->stream));
  const dim3 grid_box((unsigned)nc, std::min(grid.y, (unsigned)std::max(1, 2048 / nc)));
  hipLaunchKernelGGL(k_occ_minmax, grid_box, block, 0, s->stream, M, P, d_box);
  SSLAM_HIP_TRY(hipGetLastError());
  SSLAM_HIP_TRY(hipEventRecord(s->m_ev[1], s->stream));
  SSLAM_HIP_TRY(hipMemcpyAsync(h_box, d_box, 10 * sizeof(int), hipMemcpyDeviceToHost, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  if ((rc = occ_pass_ms(s, st, 0))) return rc;
  if (h_box[9] > 0)
    return set_error(SSLAM_ERR_UNSUPPORTED, "occupancy map: %d rays start or end beyond 2^19 cells of %g m from the map's origin", h_box[9], (double)p->resolution);
  st.n_rays = h_box[6]; st.n_truncated = h_box[7]; st.n_clipped_z = h_box[8];
  if (stats) *stats = st;
  if (st.n_rays == 0) return 0;
  // the cells are exact as floats (below 2^19), so with a leaf of 1 voxel_geometry's floorf(lo * inv) gives them back: its limits, its messages
  const float lo[3] = {(float)h_box[0], (float)h_box[1], (float)h_box[2]}, hi[3] = {(float)h_box[3], (float)h_box[4], (float)h_box[5]};
  VoxelGeom& G = F.G;
  long long* div = F.div, nbrick = 0;
  if ((rc = voxel_geometry(lo, hi, 1.0f, &G, div, &nbrick, 3))) return rc;
  G.mul[0] = 1; G.mul[1] = (int)div[0]; G.mul[2] = (int)(div[0] * div[1]);
  // pass 1: the touched bricks, their ascending list and the brick -> slot table
  const int max_bricks = 1 << 20;
  unsigned char* d_flag = nullptr; int *d_blk = nullptr;
  int *&d_list = F.d_list, *&d_slot = F.d_slot, *&d_total = F.d_total;
  const int cap_bricks = (int)std::min<long long>(nbrick, max_bricks);
  if ((rc = g.alloc(&d_flag, (size_t)nbrick)) || (rc = g.alloc(&d_list, (size_t)cap_bricks)) || (rc = g.alloc(&d_slot, (size_t)nbrick)) ||
      (rc = g.alloc(&d_blk, (size_t)((nbrick + 255) / 256))) || (rc = g.alloc(&d_total, 1))) return rc;
  SSLAM_HIP_TRY(hipMemsetAsync(d_flag, 0, (size_t)nbrick, s->stream));
  SSLAM_HIP_TRY(hipEventRecord(s->m_ev[2], s->stream));
  hipLaunchKernelGGL(k_occ_flag_bricks, grid, block, 0, s->stream, M, P, G, d_flag);
  int nocc = 0;
  if ((rc = compact_if(s, OccBrickPred{d_flag, d_list, d_slot, cap_bricks}, (int)nbrick, d_blk, d_total, nullptr, true))) return rc;
  SSLAM_HIP_TRY(hipEventRecord(s->m_ev[3], s->stream));
  SSLAM_HIP_TRY(hipMemcpyAsync(&nocc, d_total, sizeof(int), hipMemcpyDeviceToHost, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  if ((rc = occ_pass_ms(s, st, 1))) return rc;
  if (nocc > max_bricks)
    return set_error(SSLAM_ERR_UNSUPPORTED, "occupancy map: %d touched bricks of 8 x 8 x 8 cells, more than 2^20: resolution %g is too fine for these rays", nocc, (double)p->resolution);
  st.n_bricks = F.nocc = nocc;
  return 1;
}
// pass 3: the known cells that pass emit, in ascending slot * 512 + local, and their records; then the copies back, the times of passes 2
// (pass2_ms: the caller's rule) and 3, and the stats.  pred: the predicate over the cell tables, its emit / out / max_out set here;
// launch_emit(d_cells, m, d_oc, d_oh, d_om, d_ol) writes the m records.  Returns the number of records that pass emit.
template <class Pred, class Emit, class Pass2>
int occ_records(sslam_seg* s, DevGuard& g, OccFront& F, const sslam_occ_params* p, Pred pred, Emit&& launch_emit, Pass2&& pass2_ms, int32_t* cells_out,
                int32_t* hits_out, int32_t* misses_out, float* logodds_out, int max_out, sslam_occ_stats* stats) {
  int rc;
  sslam_occ_stats& st = F.st;
  int* const d_box = F.d_box;
  const size_t ncell = (size_t)F.nocc * 512;
  const int cap_list = (int)std::min<size_t>(ncell, (size_t)max_out);
  const int nblk = (int)((ncell + 255) / 256);
  int *d_cells = nullptr, *d_vblk = nullptr;
  if ((rc = g.alloc(&d_cells, (size_t)cap_list)) || (rc = g.alloc(&d_vblk, (size_t)nblk))) return rc;
  SSLAM_HIP_TRY(hipEventRecord(s->m_ev[6], s->stream));
  int total = 0;
  if (p->emit != 0) {   // n_cells counts before emit; it is read with n_steps at the end
    pred.emit = 0; pred.out = nullptr; pred.max_out = 0;
    hipLaunchKernelGGL(k_count_if<Pred>, dim3((unsigned)nblk), dim3(256), 0, s->stream, pred, (int)ncell, d_vblk);
    hipLaunchKernelGGL(k_exclusive_scan_wide, dim3(1), dim3(1024), 0, s->stream, d_vblk, nblk, d_vblk, d_box + 10);
  }
  pred.emit = p->emit; pred.out = d_cells; pred.max_out = cap_list;
  if ((rc = compact_if(s, pred, (int)ncell, d_vblk, F.d_total, &total, true))) return rc;
  const int m = std::min(total, cap_list);
  int *d_oc = nullptr, *d_oh = nullptr, *d_om = nullptr; float* d_ol = nullptr;
  if (m > 0) {
    if ((rc = g.alloc(&d_oc, (size_t)m * 3)) || (rc = g.alloc(&d_oh, (size_t)m)) || (rc = g.alloc(&d_om, (size_t)m)) || (rc = g.alloc(&d_ol, (size_t)m))) return rc;
    launch_emit(d_cells, m, d_oc, d_oh, d_om, d_ol);
    SSLAM_HIP_TRY(hipGetLastError());
  }
  SSLAM_HIP_TRY(hipEventRecord(s->m_ev[7], s->stream));
  int tail[4] = {0, 0, 0, 0};   // n_cells, -, n_steps (64 bits): waited for below, and on an error return by the guard's hipFree before this frame ends
  SSLAM_HIP_TRY(hipMemcpyAsync(tail, d_box + 10, sizeof tail, hipMemcpyDeviceToHost, s->stream));
  if (m > 0) {
    if (cells_out) SSLAM_HIP_TRY(hipMemcpyAsync(cells_out, d_oc, (size_t)m * 3 * sizeof(int), hipMemcpyDeviceToHost, s->stream));
    if (hits_out) SSLAM_HIP_TRY(hipMemcpyAsync(hits_out, d_oh, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, s->stream));
    if (misses_out) SSLAM_HIP_TRY(hipMemcpyAsync(misses_out, d_om, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, s->stream));
    if (logodds_out) SSLAM_HIP_TRY(hipMemcpyAsync(logodds_out, d_ol, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  }
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  if ((rc = pass2_ms()) || (rc = occ_pass_ms(s, st, 3))) return rc;
  st.n_cells = p->emit != 0 ? tail[0] : total;
  std::memcpy(&st.n_steps, tail + 2, sizeof st.n_steps);
  if (stats) *stats = st;
  return total;
}
}  // namespace
namespace sslam {
int seg_occupancy_map_device(sslam_seg* s, const MapCloudIn& in, const sslam_occ_params* p, int32_t* cells_out, int32_t* hits_out, int32_t* misses_out,
                             float* logodds_out, int max_out, sslam_occ_stats* stats) {
  DevGuard g;
  OccFront F{};
  int rc = occ_front(s, in, p, max_out, stats, g, F);
  if (rc <= 0) return rc;
  // pass 2: hits and misses of every cell of the touched bricks
  const size_t ncell = (size_t)F.nocc * 512;
  int *d_hits = nullptr, *d_misses = nullptr;
  if ((rc = g.alloc(&d_hits, ncell)) || (rc = g.alloc(&d_misses, ncell))) return rc;
  SSLAM_HIP_TRY(hipMemsetAsync(d_hits, 0, ncell * sizeof(int), s->stream));
  SSLAM_HIP_TRY(hipMemsetAsync(d_misses, 0, ncell * sizeof(int), s->stream));
  SSLAM_HIP_TRY(hipEventRecord(s->m_ev[4], s->stream));
  hipLaunchKernelGGL(k_occ_accumulate, F.grid, dim3(256), 0, s->stream, F.M, F.P, F.G, F.d_slot, d_hits, d_misses, (unsigned long long*)(F.d_box + 12));
  SSLAM_HIP_TRY(hipGetLastError());
  SSLAM_HIP_TRY(hipEventRecord(s->m_ev[5], s->stream));
  return occ_records(s, g, F, p, OccCellPred{d_hits, d_misses, F.L, 0, nullptr, 0},
                     [&](const int* d_cells, int m, int* d_oc, int* d_oh, int* d_om, float* d_ol) {
                       hipLaunchKernelGGL(k_occ_emit, dim3((m + 255) / 256), dim3(256), 0, s->stream, d_cells, m, F.d_list, F.G, (int)F.div[0], (int)F.div[1], d_hits,
                                          d_misses, F.L, d_oc, d_oh, d_om, d_ol);
                     },
                     [&]() { return occ_pass_ms(s, F.st, 2); }, cells_out, hits_out, misses_out, logodds_out, max_out, stats);
}

// The scan entry.  Pass 2 is a loop over chunks of kOccScanW clouds, mark then fold, all on the handle's stream with no host round trip
// in between; 2 * chunks + 1 events time the launches.
int seg_occupancy_map_scans_device(sslam_seg* s, const MapCloudIn& in, const sslam_occ_params* p, int32_t* cells_out, int32_t* hits_out,
                                   int32_t* misses_out, float* logodds_out, int max_out, sslam_occ_stats* stats) {
  if (s) { s->occ_scan_ms[0] = s->occ_scan_ms[1] = 0; s->occ_scan_counts[0] = s->occ_scan_counts[1] = 0; }
  DevGuard g;
  OccFront F{};
  int rc = occ_front(s, in, p, max_out, stats, g, F);
  if (rc <= 0) return rc;
  const int nc = in.n_clouds, nchunk = (nc + kOccScanW - 1) / kOccScanW;
  const size_t ncell = (size_t)F.nocc * 512;
  int *d_hits = nullptr, *d_misses = nullptr, *d_touched = nullptr; float* d_lo = nullptr;
  OccMask *d_hmask = nullptr, *d_mmask = nullptr; unsigned long long* d_counts = nullptr;
  if ((rc = g.alloc(&d_hits, ncell)) || (rc = g.alloc(&d_misses, ncell)) || (rc = g.alloc(&d_lo, ncell)) || (rc = g.alloc(&d_hmask, ncell)) ||
      (rc = g.alloc(&d_mmask, ncell)) || (rc = g.alloc(&d_touched, (size_t)F.nocc)) || (rc = g.alloc(&d_counts, 2))) return rc;
  while (s->occ_scan_ev.size() < 2 * (size_t)nchunk + 1) {
    hipEvent_t e = nullptr;
    SSLAM_HIP_TRY(hipEventCreate(&e));
    s->occ_scan_ev.push_back(e);
  }
  SSLAM_HIP_TRY(hipMemsetAsync(d_hits, 0, ncell * sizeof(int), s->stream));
  SSLAM_HIP_TRY(hipMemsetAsync(d_misses, 0, ncell * sizeof(int), s->stream));
  SSLAM_HIP_TRY(hipMemsetAsync(d_lo, 0, ncell * sizeof(float), s->stream));          // 0.0f
  SSLAM_HIP_TRY(hipMemsetAsync(d_hmask, 0, ncell * sizeof(OccMask), s->stream));
  SSLAM_HIP_TRY(hipMemsetAsync(d_mmask, 0, ncell * sizeof(OccMask), s->stream));
  SSLAM_HIP_TRY(hipMemsetAsync(d_touched, 0, (size_t)F.nocc * sizeof(int), s->stream));
  SSLAM_HIP_TRY(hipMemsetAsync(d_counts, 0, 2 * sizeof(unsigned long long), s->stream));
  SSLAM_HIP_TRY(hipEventRecord(s->occ_scan_ev[0], s->stream));
  for (int k = 0; k < nchunk; ++k) {
    const int base = k * kOccScanW, tag = k + 1;
    hipLaunchKernelGGL(k_occ_scan_mark, dim3((unsigned)std::min(kOccScanW, nc - base), F.grid.y), dim3(256), 0, s->stream, F.M, F.P, F.G, F.d_slot, base, tag,
                       d_hmask, d_mmask, d_touched, d_counts);
    SSLAM_HIP_TRY(hipEventRecord(s->occ_scan_ev[2 * k + 1], s->stream));
    hipLaunchKernelGGL(k_occ_scan_fold, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, s->stream, (int)ncell,
                       SSLAM_OCC_SCAN_FOLD_ALL ? (const int*)nullptr : (const int*)d_touched, tag, d_hmask, d_mmask, d_hits, d_misses, d_lo, F.L);
    if (k == nchunk - 1)   // n_steps, inside the last fold's time
      hipLaunchKernelGGL(k_occ_scan_updates, dim3((unsigned)std::min<size_t>((ncell + 255) / 256, 1024)), dim3(256), 0, s->stream, (int)ncell, d_hits, d_misses,
                         (unsigned long long*)(F.d_box + 12));
    SSLAM_HIP_TRY(hipEventRecord(s->occ_scan_ev[2 * k + 2], s->stream));
  }
  SSLAM_HIP_TRY(hipGetLastError());
  unsigned long long h_counts[2] = {0, 0};   // waited for by the records' synchronisation below, before pass2 reads it
  SSLAM_HIP_TRY(hipMemcpyAsync(h_counts, d_counts, sizeof h_counts, hipMemcpyDeviceToHost, s->stream));
  auto pass2 = [&]() -> int {
    for (int k = 0; k < 2 * nchunk; ++k) {
      float ms = 0.0f;
      SSLAM_HIP_TRY(hipEventElapsedTime(&ms, s->occ_scan_ev[k], s->occ_scan_ev[k + 1]));
      s->occ_scan_ms[k & 1] += (double)ms;
    }
    s->occ_pass_ms[2] = s->occ_scan_ms[0] + s->occ_scan_ms[1];
    F.st.kernel_ms += s->occ_pass_ms[2];
    s->occ_scan_counts[0] = (int64_t)h_counts[0]; s->occ_scan_counts[1] = (int64_t)h_counts[1];
    return 0;
  };
  return occ_records(s, g, F, p, OccScanCellPred{d_hits, d_misses, d_lo, p->l_occ, 0, nullptr, 0},
                     [&](const int* d_cells, int m, int* d_oc, int* d_oh, int* d_om, float* d_ol) {
                       hipLaunchKernelGGL(k_occ_scan_emit, dim3((m + 255) / 256), dim3(256), 0, s->stream, d_cells, m, F.d_list, F.G, (int)F.div[0], (int)F.div[1],
                                          d_hits, d_misses, d_lo, d_oc, d_oh, d_om, d_ol);
                     },
                     pass2, cells_out, hits_out, misses_out, logodds_out, max_out, stats);
}
}  // namespace sslam
extern "C" {

void sslam_occ_default_params(sslam_occ_params* p) {
  if (!p) return;
  auto logodds = [](double prob) { return (float)std::log(prob / (1.0 - prob)); };
  *p = sslam_occ_params{0.05f, 10.0f, -1.0f, 5.0f, {0.0f, 0.0f, 0.0f}, logodds(0.7), logodds(0.4), logodds(0.1192), logodds(0.971), logodds(0.5), 0};
}

// sslam_seg_occupancy_map and sslam_seg_occupancy_map_scans: the same checks and staging in front of their device entries
typedef int (*OccDeviceEntry)(sslam_seg*, const MapCloudIn&, const sslam_occ_params*, int32_t*, int32_t*, int32_t*, float*, int, sslam_occ_stats*);
static int occupancy_map_staged(OccDeviceEntry entry, sslam_seg* s, const float* xyz, const int32_t* cloud_start, int n_clouds, const double* T,
                                const sslam_occ_params* p, int32_t* cells_out, int32_t* hits_out, int32_t* misses_out, float* logodds_out, int max_out,
                                sslam_occ_stats* stats) {
  if (!s) return set_error(SSLAM_ERR_INVALID, "bad argument");
  int n_points = 0, rc;
  if ((rc = map_check_clouds("occupancy map", xyz, cloud_start, n_clouds, T, &n_points))) return rc;
  MapCloudIn in{nullptr, nullptr, nullptr, cloud_start, n_clouds};
  if (n_points == 0) return entry(s, in, p, cells_out, hits_out, misses_out, logodds_out, max_out, stats);   // the checks, then 0
  // the argument checks of the device entry come before anything is staged
  if ((rc = occupancy_check_args(p, max_out))) return rc;
  if (s->q_busy || s->n_inflight > 0) return set_error(SSLAM_ERR_INVALID, "a batch is in flight: collect it first");
  if ((rc = seg_device(s))) return rc;
  DevGuard g;
  int64_t bytes = 0;
  if ((rc = map_stage_clouds(s, g, xyz, cloud_start, n_clouds, T, n_points, &in, &bytes))) return rc;
  rc = entry(s, in, p, cells_out, hits_out, misses_out, logodds_out, max_out, stats);
  if (stats) stats->upload_bytes = bytes;
  return rc;
}

int sslam_seg_occupancy_map(sslam_seg* s, const float* xyz, const int32_t* cloud_start, int n_clouds, const double* T, const sslam_occ_params* p,
                            int32_t* cells_out, int32_t* hits_out, int32_t* misses_out, float* logodds_out, int max_out, sslam_occ_stats* stats) {
  return occupancy_map_staged(seg_occupancy_map_device, s, xyz, cloud_start, n_clouds, T, p, cells_out, hits_out, misses_out, logodds_out, max_out, stats);
}

int sslam_seg_occupancy_map_scans(sslam_seg* s, const float* xyz, const int32_t* cloud_start, int n_clouds, const double* T, const sslam_occ_params* p,
                                  int32_t* cells_out, int32_t* hits_out, int32_t* misses_out, float* logodds_out, int max_out, sslam_occ_stats* stats) {
  return occupancy_map_staged(seg_occupancy_map_scans_device, s, xyz, cloud_start, n_clouds, T, p, cells_out, hits_out, misses_out, logodds_out, max_out, stats);
}

int sslam_seg_last_occupancy_timing(const sslam_seg* s, double ms[4]) {
  if (!s || !ms) return set_error(SSLAM_ERR_INVALID, "null argument");
  for (int k = 0; k < 4; ++k) ms[k] = s->occ_pass_ms[k];
  return 0;
}

int sslam_seg_last_occupancy_scan_timing(const sslam_seg* s, double ms[2]) {
  if (!s || !ms) return set_error(SSLAM_ERR_INVALID, "null argument");
  ms[0] = s->occ_scan_ms[0]; ms[1] = s->occ_scan_ms[1];
  return 0;
}

int sslam_seg_last_occupancy_scan_counts(const sslam_seg* s, int64_t counts[2]) {
  if (!s || !counts) return set_error(SSLAM_ERR_INVALID, "null argument");
  counts[0] = s->occ_scan_counts[0]; counts[1] = s->occ_scan_counts[1];
  return 0;
}

// the mean distance of every one of n > 0 device points to its mean_k nearest neighbours -> d_md (-1 for a non-finite point)
static_assert(kSorMaxMeanK == kSorMaxK, "prefilter_check_params (csrc/odometry.hpp) bounds mean_k by it");
static int sor_mean_distance_device(sslam_seg* s, const float* d_pts, int n, int mean_k, float* d_md) {
  const size_t lds = (size_t)(128 * 3 + (mean_k + 1) * 128) * sizeof(float);
  hipLaunchKernelGGL(k_sor_mean_distance, dim3((n + 127) / 128), dim3(128), lds, s->stream, d_pts, n, mean_k, d_md);
  SSLAM_HIP_TRY(hipGetLastError());
  return 0;
}
// pcl::StatisticalOutlierRemoval::applyFilterIndices: the threshold from the moments of the valid mean distances (sequential double sums
// in index order); one expression for the host wrapper and the resident chain
static double sor_threshold(double sum, double sq, int valid, double stddev_mul) {
  const double mean = sum / valid, variance = (sq - sum * sum / valid) / (valid - 1.0), stddev = std::sqrt(variance);
  return mean + stddev_mul * stddev;
}
int sslam_seg_statistical_outlier_removal(sslam_seg* s, const float* xyz, int n, int mean_k, double stddev_mul, int32_t* keep_out, int max_out,
                                          float* mean_dist_out) {
  if (!s || !xyz || n < 0 || mean_k < 1 || mean_k >= kSorMaxK || (!keep_out && max_out > 0)) return set_error(SSLAM_ERR_INVALID, "bad argument (mean_k must be in [1, %d))", kSorMaxK);
  int rc = seg_device(s);
  if (rc) return rc;
  if (n == 0) return 0;
  int n_fin = 0;   // only finite points are neighbours: with fewer than mean_k + 1 of them no point has mean_k neighbours
  for (int i = 0; i < n; ++i) n_fin += std::isfinite(xyz[3 * (size_t)i]) && std::isfinite(xyz[3 * (size_t)i + 1]) && std::isfinite(xyz[3 * (size_t)i + 2]);
  if (n_fin < mean_k + 1) return set_error(SSLAM_ERR_INVALID, "fewer finite points (%d of %d) than mean_k + 1 = %d", n_fin, n, mean_k + 1);
  DevGuard g;
  float *d_pts = nullptr, *d_md = nullptr;
  if ((rc = g.alloc(&d_pts, (size_t)n * 3)) || (rc = g.alloc(&d_md, n))) return rc;
  SSLAM_HIP_TRY(hipMemcpyAsync(d_pts, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  if ((rc = sor_mean_distance_device(s, d_pts, n, mean_k, d_md))) return rc;
  std::vector<float> md(n);
  SSLAM_HIP_TRY(hipMemcpyAsync(md.data(), d_md, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  // pcl::StatisticalOutlierRemoval::applyFilterIndices: mean and standard deviation of the mean distances in double, in index order
  double sum = 0, sq = 0;
  int valid = 0;
  for (int i = 0; i < n; ++i) if (md[i] >= 0) { sum += md[i]; sq += (double)md[i] * md[i]; ++valid; }
  if (mean_dist_out) for (int i = 0; i < n; ++i) mean_dist_out[i] = md[i];
  if (valid < 2) return 0;
  const double thr = sor_threshold(sum, sq, valid, stddev_mul);
  int kept = 0;
  for (int i = 0; i < n; ++i)
    if (md[i] >= 0 && !((double)md[i] > thr)) { if (kept < max_out) keep_out[kept] = i; ++kept; }
  return kept;
}


// cv::kmeans as plane_segmentation::computeKmeans configures it (10 attempts, <= 10 iterations or a centre shift <= 0.01, random
// centres), restated with (a) centres drawn uniformly in the bounding box from splitmix64(seed, attempt, centre, coordinate) instead
// of cv::RNG, (b) order-independent fixed-point sums in the centre update, (c) an empty cluster keeping its centre.
int sslam_seg_kmeans(sslam_seg* s, const float* pts, int n, int dim, int k, uint64_t seed, int32_t* labels_out, float* centers_out, double* compactness_out) {
  if (!s || !pts || !labels_out || !centers_out || n <= 0 || (dim != 1 && dim != 3) || k < 1 || k > kKmMaxK) return set_error(SSLAM_ERR_INVALID, "bad argument (dim 1 or 3, 1 <= k <= %d)", kKmMaxK);
  int rc = seg_device(s);
  if (rc) return rc;
  for (size_t t = 0; t < (size_t)n * dim; ++t) if (!std::isfinite(pts[t])) return set_error(SSLAM_ERR_INVALID, "k-means input holds a non-finite value (the reference removes them first, removeNans)");
  float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (int d = 0; d < dim; ++d) { lo[d] = hi[d] = pts[d]; }
  for (int i = 1; i < n; ++i) for (int d = 0; d < dim; ++d) { const float v = pts[(size_t)i * dim + d]; lo[d] = std::min(lo[d], v); hi[d] = std::max(hi[d], v); }
  DevGuard g;
  float* d_pts = nullptr; int *d_lab = nullptr, *d_cnt = nullptr; long long *d_sums = nullptr, *d_cmp = nullptr;
  if ((rc = g.alloc(&d_pts, (size_t)n * dim)) || (rc = g.alloc(&d_lab, n)) || (rc = g.alloc(&d_cnt, kKmMaxK)) || (rc = g.alloc(&d_sums, kKmMaxK * 3)) || (rc = g.alloc(&d_cmp, 1))) return rc;
  SSLAM_HIP_TRY(hipMemcpyAsync(d_pts, pts, (size_t)n * dim * sizeof(float), hipMemcpyHostToDevice, s->stream));
  auto mix = [](uint64_t x) { x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; return x ^ (x >> 31); };
  const int attempts = 10, max_count = 10;
  const double eps2 = 0.01 * 0.01;
  double best = 1.7976931348623157e308;
  std::vector<int32_t> lab(n);
  KmCenters C; C.k = k; C.dim = dim;
  long long h_sums[kKmMaxK * 3]; int h_cnt[kKmMaxK]; long long h_cmp = 0;
  bool have = false;
  for (int a = 0; a < attempts; ++a) {
    double max_shift = 1.7976931348623157e308, compact = 0;
    bool assigned = false;
    for (int iter = 0;;) {
      if (iter == 0) {
        for (int j = 0; j < k; ++j)
          for (int d = 0; d < 3; ++d) {
            const float u = (float)(mix(seed ^ ((uint64_t)a << 40) ^ ((uint64_t)j << 20) ^ (uint64_t)d) >> 40) / 16777216.0f;
            C.c[j * 3 + d] = d < dim ? lo[d] + u * (hi[d] - lo[d]) : 0.0f;
          }
      } else {   // means of the clusters of the last assignment
        max_shift = 0;
        for (int j = 0; j < k; ++j) {
          double sh = 0;
          for (int d = 0; d < dim; ++d) {
            const float old = C.c[j * 3 + d];
            if (h_cnt[j] > 0) C.c[j * 3 + d] = (float)(((double)h_sums[j * 3 + d] / 1048576.0) / (double)h_cnt[j]);
            const double t = (double)C.c[j * 3 + d] - (double)old;
            sh += t * t;
          }
          max_shift = std::max(max_shift, sh);
        }
      }
      if (++iter == std::max(max_count, 2) || max_shift <= eps2) break;
      SSLAM_HIP_TRY(hipMemsetAsync(d_sums, 0, sizeof(long long) * kKmMaxK * 3, s->stream));
      SSLAM_HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(int) * kKmMaxK, s->stream));
      SSLAM_HIP_TRY(hipMemsetAsync(d_cmp, 0, sizeof(long long), s->stream));
      hipLaunchKernelGGL(k_kmeans_assign, dim3((n + 255) / 256), dim3(256), 0, s->stream, d_pts, n, C, d_lab, d_sums, d_cnt, d_cmp);
      SSLAM_HIP_TRY(hipGetLastError());
      SSLAM_HIP_TRY(hipMemcpyAsync(h_sums, d_sums, sizeof h_sums, hipMemcpyDeviceToHost, s->stream));
      SSLAM_HIP_TRY(hipMemcpyAsync(h_cnt, d_cnt, sizeof h_cnt, hipMemcpyDeviceToHost, s->stream));
      SSLAM_HIP_TRY(hipMemcpyAsync(&h_cmp, d_cmp, sizeof h_cmp, hipMemcpyDeviceToHost, s->stream));
      SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
      compact = (double)h_cmp / 1048576.0;
      assigned = true;
    }
    if (assigned && compact < best) {   // cv::kmeans keeps the labels of the last assignment and the centres updated after it
      best = compact;
      SSLAM_HIP_TRY(hipMemcpy(lab.data(), d_lab, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
      for (int j = 0; j < k; ++j) for (int d = 0; d < dim; ++d) centers_out[j * dim + d] = C.c[j * 3 + d];
      have = true;
    }
  }
  if (!have) return set_error(SSLAM_ERR_NUMERIC, "k-means made no assignment");
  for (int i = 0; i < n; ++i) labels_out[i] = lab[i];
  if (compactness_out) *compactness_out = best;
  return k;
}


// ---- fitness scores (k_nn_pairs, k_nn_finish) and the information matrix of a score -----------------------------------------------

// SSLAM_FITNESS_OPTS="chunk=N": targets per workgroup of k_nn_pairs (0: the heuristic).  Read at each call: tests toggle it.
static int fitness_chunk_from_env() {
  const char* e = getenv("SSLAM_FITNESS_OPTS");
  if (!e) return 0;
  const char* c = strstr(e, "chunk=");
  if (!c) return 0;
  const long v = strtol(c + 6, nullptr, 10);
  return v > 0 && v < (1l << 30) ? (int)v : 0;
}

// The host side of a nearest-neighbour pass, shared by sslam_seg_fitness_scores and sslam_seg_register_pairs: the checks of the cloud
// layout, the plan (pairs as the kernels read them, items, runs), the device buffers and the two halves of the pass.
static int nn_check_clouds(const float* xyz, const int32_t* cloud_start, int n_clouds, const sslam_fitness_pair* pairs, int n_pairs) {
  if (cloud_start[0] < 0) return set_error(SSLAM_ERR_INVALID, "cloud_start[0] is negative");
  for (int c = 0; c < n_clouds; ++c)
    if (cloud_start[c + 1] < cloud_start[c]) return set_error(SSLAM_ERR_INVALID, "cloud_start decreases at cloud %d", c);
  if (cloud_start[n_clouds] > 0 && !xyz) return set_error(SSLAM_ERR_INVALID, "null xyz");
  for (int p = 0; p < n_pairs; ++p)
    if (pairs[p].target < 0 || pairs[p].target >= n_clouds || pairs[p].source < 0 || pairs[p].source >= n_clouds)
      return set_error(SSLAM_ERR_INVALID, "pair %d names cloud %d / %d of %d", p, pairs[p].target, pairs[p].source, n_clouds);
  return 0;
}
struct NnPlan {
  std::vector<NnPair> hp;
  std::vector<NnItem> items;
  std::vector<NnSeg> segs;
  long long total_q = 0;
};
struct NnDev {
  float *xyz = nullptr, *d2 = nullptr;
  NnPair* pairs = nullptr; NnItem* items = nullptr; NnSeg* segs = nullptr;
  unsigned long long* best = nullptr;
  int *idx = nullptr, *used = nullptr;
  double* sum = nullptr;
};
static int nn_plan(sslam_seg* s, const int32_t* cloud_start, const sslam_fitness_pair* pairs, int n_pairs, NnPlan& pl) {
  if (!s->n_cu) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, s->P.device) != hipSuccess || v <= 0) v = 256;
    s->n_cu = v;
  }
  // the pairs as the kernels read them, the source blocks (items before the target split) and the runs of the reduction
  std::vector<NnPair>& hp = pl.hp;
  hp.resize(n_pairs);
  long long total_q = 0, blocks = 0, n_seg = 0;
  for (int p = 0; p < n_pairs; ++p) {
    NnPair& P = hp[p];
    P.t0 = cloud_start[pairs[p].target]; P.nt = cloud_start[pairs[p].target + 1] - P.t0;
    P.s0 = cloud_start[pairs[p].source]; P.ns = cloud_start[pairs[p].source + 1] - P.s0;
    P.qoff = total_q;
    for (int k = 0; k < 9; ++k) P.R[k] = (float)pairs[p].T[k];
    for (int k = 0; k < 3; ++k) P.t[k] = (float)pairs[p].T[9 + k];
    P.max_range = pairs[p].max_range;
    total_q += P.ns;
    if (P.nt > 0) blocks += (P.ns + kNnQ - 1) / kNnQ;
    n_seg += (P.ns + kNnSeg - 1) / kNnSeg;
  }
  pl.total_q = total_q;
  // Target split.  Without it the launch has `blocks` workgroups; below four per compute unit the targets of every pair are cut into
  // as many chunks as bring it there, never shorter than two tiles (a workgroup should scan long enough to pay for its query loads
  // and atomics).  Chunk boundaries do not change any result.
  int chunk = fitness_chunk_from_env();
  long long split = 1;
  if (!chunk && blocks > 0 && blocks < 4ll * s->n_cu) split = (4ll * s->n_cu + blocks - 1) / blocks;
  std::vector<NnItem>& items = pl.items;
  std::vector<NnSeg>& segs = pl.segs;
  segs.reserve((size_t)n_seg);
  for (int p = 0; p < n_pairs; ++p) {
    const NnPair& P = hp[p];
    for (int g = 0; g < (P.ns + kNnSeg - 1) / kNnSeg; ++g) segs.push_back(NnSeg{p, g});
    if (P.nt <= 0 || P.ns <= 0) continue;
    long long ch = chunk;
    if (!ch) {
      ch = (P.nt + split - 1) / split;
      ch = std::max<long long>((ch + kNnTile - 1) / kNnTile * kNnTile, 2 * kNnTile);
    }
    const long long nch = (P.nt + ch - 1) / ch, nqb = (P.ns + kNnQ - 1) / kNnQ;
    if ((long long)items.size() + nch * nqb > (1ll << 24))
      return set_error(SSLAM_ERR_UNSUPPORTED, "fitness pass of more than 2^24 workgroups (chunk = %lld targets is too small for these clouds)", ch);
    for (long long qb = 0; qb < nqb; ++qb)
      for (long long c = 0; c < nch; ++c)
        items.push_back(NnItem{p, (int)qb, (int)(c * ch), (int)std::min<long long>((c + 1) * ch, P.nt)});
  }
  return 0;
}
// buffers and the copies to the device, all on the handle's stream; f_e0 is NOT recorded here.  With d.xyz set by the caller the points
// already sit on the device (the odometry's arena): xyz is not read and nothing is allocated for them.
static int nn_upload(sslam_seg* s, DevGuard& g, const NnPlan& pl, const float* xyz, int n_points, NnDev& d) {
  int rc;
  const size_t total_q = (size_t)pl.total_q;
  const bool resident = d.xyz != nullptr;
  if ((!resident && (rc = g.alloc(&d.xyz, (size_t)n_points * 3))) || (rc = g.alloc(&d.pairs, pl.hp.size())) || (rc = g.alloc(&d.items, pl.items.size())) ||
      (rc = g.alloc(&d.segs, pl.segs.size())) || (rc = g.alloc(&d.best, total_q)) || (rc = g.alloc(&d.idx, total_q)) ||
      (rc = g.alloc(&d.d2, total_q)) || (rc = g.alloc(&d.sum, pl.segs.size())) || (rc = g.alloc(&d.used, pl.segs.size()))) return rc;
  if (!s->f_e0) { SSLAM_HIP_TRY(hipEventCreate(&s->f_e0)); SSLAM_HIP_TRY(hipEventCreate(&s->f_e1)); }
  if (!resident && n_points > 0) SSLAM_HIP_TRY(hipMemcpyAsync(d.xyz, xyz, (size_t)n_points * 3 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  SSLAM_HIP_TRY(hipMemcpyAsync(d.pairs, pl.hp.data(), pl.hp.size() * sizeof(NnPair), hipMemcpyHostToDevice, s->stream));
  if (!pl.items.empty()) SSLAM_HIP_TRY(hipMemcpyAsync(d.items, pl.items.data(), pl.items.size() * sizeof(NnItem), hipMemcpyHostToDevice, s->stream));
  if (!pl.segs.empty()) SSLAM_HIP_TRY(hipMemcpyAsync(d.segs, pl.segs.data(), pl.segs.size() * sizeof(NnSeg), hipMemcpyHostToDevice, s->stream));
  return 0;
}
// reset `best` and search: the nearest target of every source point at the R, t the device's pair table holds
static int nn_search(sslam_seg* s, const NnPlan& pl, const NnDev& d) {
  if (pl.total_q > 0) SSLAM_HIP_TRY(hipMemsetAsync(d.best, 0xff, (size_t)pl.total_q * sizeof(unsigned long long), s->stream));
  if (!pl.items.empty()) hipLaunchKernelGGL(k_nn_pairs, dim3((unsigned)pl.items.size()), dim3(kNnThreads), 0, s->stream, d.xyz, d.pairs, d.items, d.best);
  return 0;
}
// k_nn_finish, f_e1, the copies back, the wait, and the score of every pair (the time between f_e0 and f_e1 goes to kernel_ms)
static int nn_finish(sslam_seg* s, const NnPlan& pl, const NnDev& d, double* score_out, int32_t* used_out, int32_t* nn_index_out, float* nn_dist2_out,
                     double* kernel_ms) {
  const std::vector<NnSeg>& segs = pl.segs;
  const size_t total_q = (size_t)pl.total_q;
  if (!segs.empty()) hipLaunchKernelGGL(k_nn_finish, dim3((unsigned)segs.size()), dim3(kNnSeg), 0, s->stream, d.pairs, d.segs, d.best, d.idx, d.d2, d.sum, d.used);
  SSLAM_HIP_TRY(hipGetLastError());
  SSLAM_HIP_TRY(hipEventRecord(s->f_e1, s->stream));
  std::vector<double> h_sum(segs.size());
  std::vector<int> h_used(segs.size());
  if (!segs.empty()) {
    SSLAM_HIP_TRY(hipMemcpyAsync(h_sum.data(), d.sum, segs.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    SSLAM_HIP_TRY(hipMemcpyAsync(h_used.data(), d.used, segs.size() * sizeof(int), hipMemcpyDeviceToHost, s->stream));
  }
  if (total_q > 0 && nn_index_out) SSLAM_HIP_TRY(hipMemcpyAsync(nn_index_out, d.idx, total_q * sizeof(int), hipMemcpyDeviceToHost, s->stream));
  if (total_q > 0 && nn_dist2_out) SSLAM_HIP_TRY(hipMemcpyAsync(nn_dist2_out, d.d2, total_q * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  if (kernel_ms) {
    float ms = 0.0f;
    SSLAM_HIP_TRY(hipEventElapsedTime(&ms, s->f_e0, s->f_e1));
    *kernel_ms = (double)ms;
  }
  size_t at = 0;
  for (size_t p = 0; p < pl.hp.size(); ++p) {   // the runs of a pair in ascending order
    double sum = 0.0;
    long long used = 0;
    for (int k = 0; k < (pl.hp[p].ns + kNnSeg - 1) / kNnSeg; ++k, ++at) { sum += h_sum[at]; used += h_used[at]; }
    used_out[p] = (int32_t)used;
    score_out[p] = used > 0 ? sum / (double)used : 1.7976931348623157e308;
  }
  return 0;
}

int sslam_seg_fitness_scores(sslam_seg* s, const float* xyz, const int32_t* cloud_start, int n_clouds, const sslam_fitness_pair* pairs, int n_pairs,
                             double* score_out, int32_t* used_out, int32_t* nn_index_out, float* nn_dist2_out, double* kernel_ms) {
  if (!s || !cloud_start || n_clouds < 0 || n_pairs < 0 || (n_pairs > 0 && (!pairs || !score_out || !used_out)))
    return set_error(SSLAM_ERR_INVALID, "bad argument");
  int rc = nn_check_clouds(xyz, cloud_start, n_clouds, pairs, n_pairs);
  if (rc) return rc;
  if (s->q_busy || s->n_inflight > 0) return set_error(SSLAM_ERR_INVALID, "a batch is in flight: collect it first");
  rc = seg_device(s);
  if (rc) return rc;
  if (kernel_ms) *kernel_ms = 0.0;
  if (n_pairs == 0) return 0;
  NnPlan pl;
  if ((rc = nn_plan(s, cloud_start, pairs, n_pairs, pl))) return rc;
  DevGuard g;
  NnDev d;
  if ((rc = nn_upload(s, g, pl, xyz, cloud_start[n_clouds], d))) return rc;
  SSLAM_HIP_TRY(hipEventRecord(s->f_e0, s->stream));
  if ((rc = nn_search(s, pl, d)) || (rc = nn_finish(s, pl, d, score_out, used_out, nn_index_out, nn_dist2_out, kernel_ms))) return rc;
  return n_pairs;
}

// ---- per-point covariances of generalized ICP (k_knn_cov) ----------------------------------------------------------------------------
void sslam_gicp_default_params(sslam_gicp_params* p) {
  if (!p) return;
  p->k = 20; p->plane_epsilon = 1e-3;   // fast_gicp's k_correspondences and its PLANE regularisation [UPSTREAM, quoted from memory]
}
// k_knn_cov over the clouds that `wanted` marks (NULL: all) of the device's point table: the block table goes up, one launch; with
// `timed`, f_e0 and f_e1 are recorded right before and right after the launch (nothing but the kernel lies between them)
static int knn_cov_launch(sslam_seg* s, DevGuard& g, const float* d_xyz, const int32_t* cloud_start, int n_clouds, const unsigned char* wanted, int k,
                          double plane_epsilon, double* d_cov, int* d_knn, bool timed) {
  std::vector<KnnBlock> blocks;
  for (int c = 0; c < n_clouds; ++c) {
    if (wanted && !wanted[c]) continue;
    const int n = cloud_start[c + 1] - cloud_start[c];
    for (int q0 = 0; q0 < n; q0 += kKnnThreads) blocks.push_back(KnnBlock{cloud_start[c], n, q0});
  }
  if (blocks.empty()) {
    if (timed) { SSLAM_HIP_TRY(hipEventRecord(s->f_e0, s->stream)); SSLAM_HIP_TRY(hipEventRecord(s->f_e1, s->stream)); }
    return 0;
  }
  KnnBlock* d_blocks = nullptr;
  int rc;
  if ((rc = g.alloc(&d_blocks, blocks.size()))) return rc;
  SSLAM_HIP_TRY(hipMemcpyAsync(d_blocks, blocks.data(), blocks.size() * sizeof(KnnBlock), hipMemcpyHostToDevice, s->stream));
  const size_t lds = (size_t)kKnnThreads * (3 * sizeof(float) + (size_t)k * (sizeof(float) + sizeof(int)));   // 21.5 KB at k = 20, 33.5 KB at 32
  if (timed) SSLAM_HIP_TRY(hipEventRecord(s->f_e0, s->stream));
  hipLaunchKernelGGL(k_knn_cov, dim3((unsigned)blocks.size()), dim3(kKnnThreads), lds, s->stream, d_xyz, d_blocks, k, plane_epsilon, d_cov, d_knn);
  if (timed) SSLAM_HIP_TRY(hipEventRecord(s->f_e1, s->stream));
  SSLAM_HIP_TRY(hipGetLastError());
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));   // the block table leaves scope with the caller's vector
  return 0;
}
int sslam_seg_cloud_covariances(sslam_seg* s, const float* xyz, const int32_t* cloud_start, int n_clouds, int k, double plane_epsilon, double* cov_out,
                                int32_t* knn_index_out, double* kernel_ms) {
  if (!s || !cloud_start || n_clouds < 0) return set_error(SSLAM_ERR_INVALID, "bad argument");
  int rc = nn_check_clouds(xyz, cloud_start, n_clouds, nullptr, 0);
  if (rc) return rc;
  const int n_points = cloud_start[n_clouds];
  if (n_points > 0 && !cov_out) return set_error(SSLAM_ERR_INVALID, "null cov_out");
  if ((rc = gicp_check_params(k, plane_epsilon))) return rc;
  if (s->q_busy || s->n_inflight > 0) return set_error(SSLAM_ERR_INVALID, "a batch is in flight: collect it first");
  rc = seg_device(s);
  if (rc) return rc;
  if (kernel_ms) *kernel_ms = 0.0;
  if (n_points == 0) return 0;
  DevGuard g;
  float* d_xyz = nullptr;
  double* d_cov = nullptr;
  int* d_knn = nullptr;
  if ((rc = g.alloc(&d_xyz, (size_t)n_points * 3)) || (rc = g.alloc(&d_cov, (size_t)n_points * 6)) ||
      (knn_index_out && (rc = g.alloc(&d_knn, (size_t)n_points * k)))) return rc;
  if (!s->f_e0) { SSLAM_HIP_TRY(hipEventCreate(&s->f_e0)); SSLAM_HIP_TRY(hipEventCreate(&s->f_e1)); }
  SSLAM_HIP_TRY(hipMemcpyAsync(d_xyz, xyz, (size_t)n_points * 3 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  // points before cloud_start[0] belong to no cloud: their entries are zeros
  SSLAM_HIP_TRY(hipMemsetAsync(d_cov, 0, (size_t)n_points * 6 * sizeof(double), s->stream));
  if (d_knn) SSLAM_HIP_TRY(hipMemsetAsync(d_knn, 0xff, (size_t)n_points * k * sizeof(int), s->stream));
  if ((rc = knn_cov_launch(s, g, d_xyz, cloud_start, n_clouds, nullptr, k, plane_epsilon, d_cov, d_knn, true))) return rc;
  SSLAM_HIP_TRY(hipMemcpyAsync(cov_out, d_cov, (size_t)n_points * 6 * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  if (d_knn) SSLAM_HIP_TRY(hipMemcpyAsync(knn_index_out, d_knn, (size_t)n_points * k * sizeof(int), hipMemcpyDeviceToHost, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  if (kernel_ms) {
    float ms = 0.0f;
    SSLAM_HIP_TRY(hipEventElapsedTime(&ms, s->f_e0, s->f_e1));
    *kernel_ms = (double)ms;
  }
  return n_points;
}

// ---- scan matching: nearest-neighbour ICP of cloud pairs (k_nn_pairs, k_reg_sums, k_reg_step; k_nn_finish at the end), and its
// generalized form (k_gicp_sums, k_gicp_step in their place; gp != NULL): one host loop for both ------------------------------------------
// d_xyz / d_cov_resident: NULL, or the points (and, with gp, the covariances of every cloud a pair names) where they already sit on the
// device -- the odometry's arena; xyz and cov are then not read.  Everything after the staging is the same code for both callers.
static int register_pairs(sslam_seg* s, const float* xyz, const int32_t* cloud_start, int n_clouds, const sslam_reg_pair* pairs, int n_pairs,
                          const double* cov, const sslam_gicp_params* gp, int max_iterations, double epsilon, sslam_reg_result* out,
                          int32_t* nn_index_out, float* nn_dist2_out, double* kernel_ms, float* d_xyz = nullptr, double* d_cov_resident = nullptr) {
  if (!s || !cloud_start || n_clouds < 0 || n_pairs < 0 || (n_pairs > 0 && (!pairs || !out)) || max_iterations < 0 || !(epsilon >= 0.0))
    return set_error(SSLAM_ERR_INVALID, "bad argument");
  if (gp) { const int rcp = gicp_check_params(gp->k, gp->plane_epsilon); if (rcp) return rcp; }
  std::vector<sslam_fitness_pair> fp(n_pairs);   // the search reads a pair as the fitness pass does: T = the initial guess, max_range = max_corr2
  for (int p = 0; p < n_pairs; ++p) {
    fp[p].target = pairs[p].target; fp[p].source = pairs[p].source; fp[p].max_range = pairs[p].max_corr2;
    for (int k = 0; k < 12; ++k) fp[p].T[k] = pairs[p].T0[k];
  }
  int rc = nn_check_clouds(d_xyz ? d_xyz : xyz, cloud_start, n_clouds, fp.data(), n_pairs);
  if (rc) return rc;
  if (s->q_busy || s->n_inflight > 0) return set_error(SSLAM_ERR_INVALID, "a batch is in flight: collect it first");
  rc = seg_device(s);
  if (rc) return rc;
  if (kernel_ms) *kernel_ms = 0.0;
  if (n_pairs == 0) return 0;
  NnPlan pl;
  if ((rc = nn_plan(s, cloud_start, fp.data(), n_pairs, pl))) return rc;
  std::vector<RegState> h_st(n_pairs);
  std::vector<int> seg0(n_pairs + 1, 0);       // first run of every pair in the partial records
  for (int p = 0; p < n_pairs; ++p) {
    RegState& S = h_st[p];
    for (int k = 0; k < 12; ++k) S.T[k] = pairs[p].T0[k];
    S.iterations = S.converged = S.status = S.done = 0;
    seg0[p + 1] = seg0[p] + (pl.hp[p].ns + kNnSeg - 1) / kNnSeg;
  }
  DevGuard g;
  NnDev d;
  RegState* d_st = nullptr;
  int *d_seg0 = nullptr, *d_live = nullptr;
  double* d_part = nullptr;
  const int n_sums = gp ? kIcpSums : kRegSums;
  const size_t n_points = (size_t)cloud_start[n_clouds];
  double* d_cov = d_cov_resident;
  d.xyz = d_xyz;
  if ((rc = nn_upload(s, g, pl, xyz, cloud_start[n_clouds], d)) || (rc = g.alloc(&d_st, (size_t)n_pairs)) || (rc = g.alloc(&d_seg0, seg0.size())) ||
      (rc = g.alloc(&d_live, 1)) || (rc = g.alloc(&d_part, pl.segs.size() * n_sums)) || (gp && !d_cov && (rc = g.alloc(&d_cov, n_points * 6)))) return rc;
  if (gp && !d_cov_resident && max_iterations > 0 && n_points > 0) {   // the covariances: the caller's, or those of every cloud a pair names, each cloud once
    if (cov) {
      SSLAM_HIP_TRY(hipMemcpyAsync(d_cov, cov, n_points * 6 * sizeof(double), hipMemcpyHostToDevice, s->stream));
    } else {
      std::vector<unsigned char> wanted(n_clouds, 0);
      for (int p = 0; p < n_pairs; ++p) wanted[pairs[p].target] = wanted[pairs[p].source] = 1;
      SSLAM_HIP_TRY(hipMemsetAsync(d_cov, 0, n_points * 6 * sizeof(double), s->stream));
      if ((rc = knn_cov_launch(s, g, d.xyz, cloud_start, n_clouds, wanted.data(), gp->k, gp->plane_epsilon, d_cov, nullptr, false))) return rc;
    }
  }
  int live = n_pairs;
  SSLAM_HIP_TRY(hipMemcpyAsync(d_st, h_st.data(), h_st.size() * sizeof(RegState), hipMemcpyHostToDevice, s->stream));
  SSLAM_HIP_TRY(hipMemcpyAsync(d_seg0, seg0.data(), seg0.size() * sizeof(int), hipMemcpyHostToDevice, s->stream));
  SSLAM_HIP_TRY(hipMemcpyAsync(d_live, &live, sizeof(int), hipMemcpyHostToDevice, s->stream));
  SSLAM_HIP_TRY(hipEventRecord(s->f_e0, s->stream));
  // Iterations in chunks of at most 8, no host round trip inside a chunk; between chunks the number of unfinished pairs comes back.
  // Every unfinished pair has made the same number of updates, so the cap needs no per-pair count.
  for (int it = 0; it < max_iterations && live > 0;) {
    const int n = std::min(8, max_iterations - it);
    for (int k = 0; k < n; ++k) {
      if ((rc = nn_search(s, pl, d))) return rc;
      if (gp) {
        if (!pl.segs.empty()) hipLaunchKernelGGL(k_gicp_sums, dim3((unsigned)pl.segs.size()), dim3(kNnSeg), 0, s->stream, d.xyz, d_cov, d.pairs, d.segs, d.best, d_st, d_part);
        hipLaunchKernelGGL(k_gicp_step, dim3((unsigned)n_pairs), dim3(64), 0, s->stream, d_seg0, d_part, epsilon, d.pairs, d_st, d_live);
        continue;
      }
      if (!pl.segs.empty()) hipLaunchKernelGGL(k_reg_sums, dim3((unsigned)pl.segs.size()), dim3(kNnSeg), 0, s->stream, d.xyz, d.pairs, d.segs, d.best, d_st, d_part);
      hipLaunchKernelGGL(k_reg_step, dim3((unsigned)n_pairs), dim3(64), 0, s->stream, d_seg0, d_part, epsilon, d.pairs, d_st, d_live);
    }
    SSLAM_HIP_TRY(hipGetLastError());
    SSLAM_HIP_TRY(hipMemcpyAsync(&live, d_live, sizeof(int), hipMemcpyDeviceToHost, s->stream));
    SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
    it += n;
  }
  // the fitness pass at the estimate the loop ended at: the pair table holds its float casts
  SSLAM_HIP_TRY(hipMemcpyAsync(h_st.data(), d_st, h_st.size() * sizeof(RegState), hipMemcpyDeviceToHost, s->stream));
  std::vector<double> score(n_pairs);
  std::vector<int32_t> used(n_pairs);
  if ((rc = nn_search(s, pl, d)) || (rc = nn_finish(s, pl, d, score.data(), used.data(), nn_index_out, nn_dist2_out, kernel_ms))) return rc;
  for (int p = 0; p < n_pairs; ++p) {
    const RegState& S = h_st[p];
    for (int k = 0; k < 12; ++k) out[p].T[k] = S.T[k];
    out[p].score = score[p]; out[p].used = used[p];
    out[p].iterations = S.iterations; out[p].converged = S.converged; out[p].status = S.status;
  }
  return n_pairs;
}
int sslam_seg_register_pairs(sslam_seg* s, const float* xyz, const int32_t* cloud_start, int n_clouds, const sslam_reg_pair* pairs, int n_pairs,
                             int max_iterations, double epsilon, sslam_reg_result* out, int32_t* nn_index_out, float* nn_dist2_out, double* kernel_ms) {
  return register_pairs(s, xyz, cloud_start, n_clouds, pairs, n_pairs, nullptr, nullptr, max_iterations, epsilon, out, nn_index_out, nn_dist2_out, kernel_ms);
}
int sslam_seg_register_pairs_gicp(sslam_seg* s, const float* xyz, const int32_t* cloud_start, int n_clouds, const sslam_reg_pair* pairs, int n_pairs,
                                  const double* cov, const sslam_gicp_params* params, int max_iterations, double epsilon, sslam_reg_result* out,
                                  int32_t* nn_index_out, float* nn_dist2_out, double* kernel_ms) {
  sslam_gicp_params gp;
  sslam_gicp_default_params(&gp);
  if (params) gp = *params;
  return register_pairs(s, xyz, cloud_start, n_clouds, pairs, n_pairs, cov, &gp, max_iterations, epsilon, out, nn_index_out, nn_dist2_out, kernel_ms);
}

// ---- scan-matching odometry: radius outlier removal, the resident prefilter chain, the odometry handle (kernels and host rules in
// csrc/odometry.hpp; the contract is at sslam_seg_prefilter / sslam_odom_push in include/sslam.h) ----------------------------------------
static int radius_count_device(sslam_seg* s, const float* d_pts, int n, double radius, int* d_count) {
  const float r2 = (float)(radius * radius);
  hipLaunchKernelGGL(k_radius_count, dim3((n + kRadThreads - 1) / kRadThreads), dim3(kRadThreads), 0, s->stream, d_pts, n, r2, d_count);
  SSLAM_HIP_TRY(hipGetLastError());
  return 0;
}
int sslam_seg_radius_outlier_removal(sslam_seg* s, const float* xyz, int n, double radius, int min_neighbors, int32_t* keep_out, int max_out,
                                     int32_t* count_out) {
  if (!s || !xyz || n < 0 || (!keep_out && max_out > 0) || !(radius > 0 && std::isfinite(radius)) || min_neighbors < 0)
    return set_error(SSLAM_ERR_INVALID, "bad argument (radius must be finite and positive, min_neighbors >= 0)");
  int rc = seg_device(s);
  if (rc) return rc;
  if (n == 0) return 0;
  DevGuard g;
  float* d_pts = nullptr; int *d_cnt = nullptr, *d_out = nullptr; unsigned char* d_flag = nullptr;
  if ((rc = g.alloc(&d_pts, (size_t)n * 3)) || (rc = g.alloc(&d_cnt, n)) || (rc = g.alloc(&d_flag, n)) || (rc = g.alloc(&d_out, n))) return rc;
  SSLAM_HIP_TRY(hipMemcpyAsync(d_pts, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  if ((rc = radius_count_device(s, d_pts, n, radius, d_cnt))) return rc;
  hipLaunchKernelGGL(k_radius_flag, dim3((n + 255) / 256), dim3(256), 0, s->stream, d_cnt, n, min_neighbors, d_flag);
  int total = 0;
  if ((rc = compact_flags(s, g, d_flag, n, d_out, n, &total))) return rc;
  const int m = std::min(total, max_out);
  if (m > 0) SSLAM_HIP_TRY(hipMemcpy(keep_out, d_out, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
  if (count_out) SSLAM_HIP_TRY(hipMemcpy(count_out, d_cnt, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  return total;
}

void sslam_prefilter_default_params(sslam_prefilter_params* p) {
  if (!p) return;
  memset(p, 0, sizeof *p);
  p->use_distance_filter = 1; p->distance_near = 1.0; p->distance_far = 100.0;   // hdl's prefiltering_nodelet [UPSTREAM, quoted from memory]
  p->downsample = SSLAM_DOWNSAMPLE_VOXELGRID; p->leaf = 0.1f;
  p->outlier = SSLAM_OUTLIER_STATISTICAL; p->mean_k = 20; p->stddev_mul = 1.0;
  p->radius = 0.8; p->min_neighbors = 2;
}
// The chain over n points that sit on the device (d_in is only read).  *d_res: the result, *m_out points -- a buffer of the guard's, or
// d_in itself where nothing was dropped.  Each stage's kept points go through compact_if with GatherPred: the index list of the host entry
// point and its gather in one.  `clean`: the non-finite points are gone.
static int prefilter_device(sslam_seg* s, DevGuard& g, const float* d_in, int n, const sslam_prefilter_params* p, const float** d_res, int* m_out,
                            int32_t counts[3]) {
  const float* cur = d_in;
  int m = n, rc;
  bool clean = false;
  unsigned char* d_flag = nullptr; int *d_blk = nullptr, *d_total = nullptr;
  if ((rc = g.alloc(&d_flag, n)) || (rc = g.alloc(&d_blk, (n + 255) / 256)) || (rc = g.alloc(&d_total, 1))) return rc;
  auto keep_flagged = [&]() -> int {     // m > 0
    float* dst = nullptr;
    int total = 0, rc2;
    if ((rc2 = g.alloc(&dst, (size_t)m * 3)) || (rc2 = compact_if(s, GatherPred{d_flag, cur, dst}, m, d_blk, d_total, &total))) return rc2;
    cur = dst; m = total; clean = true;
    return 0;
  };
  if (p->use_distance_filter && m > 0) {
    hipLaunchKernelGGL(k_range_flag, dim3((m + 255) / 256), dim3(256), 0, s->stream, cur, m, p->distance_near, p->distance_far, d_flag);
    if ((rc = keep_flagged())) return rc;
  }
  counts[0] = m;
  if (p->downsample == SSLAM_DOWNSAMPLE_VOXELGRID && m > 0) {
    float* d_out = nullptr; int* d_oc = nullptr;
    int nocc = 0;
    if ((rc = voxel_grid_device(s, g, cur, m, p->leaf, &d_out, &d_oc, &nocc))) return rc;
    cur = d_out; m = nocc; clean = true;
  }
  counts[1] = m;
  if (!clean && m > 0) {                 // no stage has run: the compaction of the finite points
    hipLaunchKernelGGL(k_finite_flag, dim3((m + 255) / 256), dim3(256), 0, s->stream, cur, m, d_flag);
    if ((rc = keep_flagged())) return rc;
  }
  if (p->outlier == SSLAM_OUTLIER_STATISTICAL && m >= p->mean_k + 1) {
    float* d_md = nullptr; double* d_mom = nullptr;
    double mom[3] = {0, 0, 0};
    if ((rc = g.alloc(&d_md, m)) || (rc = g.alloc(&d_mom, 3)) || (rc = sor_mean_distance_device(s, cur, m, p->mean_k, d_md))) return rc;
    hipLaunchKernelGGL(k_sor_moments, dim3(1), dim3(64), 0, s->stream, d_md, m, d_mom);
    SSLAM_HIP_TRY(hipMemcpyAsync(mom, d_mom, sizeof mom, hipMemcpyDeviceToHost, s->stream));
    SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
    const int valid = (int)mom[2];
    if (valid < 2) m = 0;                // the stand-alone call keeps nothing there
    else {
      hipLaunchKernelGGL(k_sor_flag, dim3((m + 255) / 256), dim3(256), 0, s->stream, d_md, m, sor_threshold(mom[0], mom[1], valid, p->stddev_mul), d_flag);
      if ((rc = keep_flagged())) return rc;
    }
  } else if (p->outlier == SSLAM_OUTLIER_RADIUS && m > 0) {
    int* d_cnt = nullptr;
    if ((rc = g.alloc(&d_cnt, m)) || (rc = radius_count_device(s, cur, m, p->radius, d_cnt))) return rc;
    hipLaunchKernelGGL(k_radius_flag, dim3((m + 255) / 256), dim3(256), 0, s->stream, d_cnt, m, p->min_neighbors, d_flag);
    if ((rc = keep_flagged())) return rc;
  }
  counts[2] = m;
  SSLAM_HIP_TRY(hipGetLastError());
  *d_res = cur; *m_out = m;
  return 0;
}
int sslam_seg_prefilter(sslam_seg* s, const float* xyz, int n, const sslam_prefilter_params* p, float* xyz_out, int max_out, int32_t counts[3],
                        double* kernel_ms) {
  if (!s || !p || n < 0 || (!xyz && n > 0) || max_out < 0 || (!xyz_out && max_out > 0)) return set_error(SSLAM_ERR_INVALID, "bad argument");
  int rc = prefilter_check_params(p);
  if (rc) return rc;
  if (s->q_busy || s->n_inflight > 0) return set_error(SSLAM_ERR_INVALID, "a batch is in flight: collect it first");
  if ((rc = seg_device(s))) return rc;
  if (kernel_ms) *kernel_ms = 0.0;
  int32_t cnt[3] = {0, 0, 0};
  if (counts) memcpy(counts, cnt, sizeof cnt);
  if (n == 0) return 0;
  DevGuard g;
  float* d_in = nullptr;
  const float* d_res = nullptr;
  int m = 0;
  if ((rc = g.alloc(&d_in, (size_t)n * 3))) return rc;
  if (!s->f_e0) { SSLAM_HIP_TRY(hipEventCreate(&s->f_e0)); SSLAM_HIP_TRY(hipEventCreate(&s->f_e1)); }
  SSLAM_HIP_TRY(hipMemcpyAsync(d_in, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  SSLAM_HIP_TRY(hipEventRecord(s->f_e0, s->stream));
  if ((rc = prefilter_device(s, g, d_in, n, p, &d_res, &m, cnt))) return rc;
  SSLAM_HIP_TRY(hipEventRecord(s->f_e1, s->stream));
  const int w = std::min(m, max_out);
  if (w > 0) SSLAM_HIP_TRY(hipMemcpyAsync(xyz_out, d_res, (size_t)w * 3 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  if (kernel_ms) {
    float ms = 0.0f;
    SSLAM_HIP_TRY(hipEventElapsedTime(&ms, s->f_e0, s->f_e1));
    *kernel_ms = (double)ms;
  }
  if (counts) memcpy(counts, cnt, sizeof cnt);
  return m;
}

}  // extern "C"
// The odometry handle.  The device arena holds TWO slots of `cap` points each (and, under GICP, of 6 doubles per point): the keyframe's
// filtered cloud in one, the frame's in the other, so that one base pointer serves the pair table of the registration kernels; a frame
// that becomes the keyframe swaps the roles of the slots.
struct sslam_odom {
  sslam_seg* seg = nullptr;
  sslam_odom_params P;
  bool has_kf = false;
  double kf_pose[12], prev[12];
  int32_t kf_sec = 0, kf_nsec = 0;
  float* d_xyz = nullptr;
  double* d_cov = nullptr;
  size_t cap = 0;
  int kf_slot = 0, kf_n = 0, keyframes = 0;
  int64_t cov_passes = 0;
  hipEvent_t ev[2] = {nullptr, nullptr};   // around the prefilter
  ~sslam_odom() {
    if (!d_xyz && !d_cov && !ev[0]) return;
    (void)hipSetDevice(seg_device_index(seg));
    if (d_xyz) (void)hipFree(d_xyz);
    if (d_cov) (void)hipFree(d_cov);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  }
};
// room for `need` points per slot; the keyframe's slot moves with the arena (device to device)
static int odom_reserve(sslam_odom* o, size_t need) {
  if (need <= o->cap) return 0;
  sslam_seg* s = o->seg;
  const bool gicp = o->P.method == SSLAM_REG_GICP;
  const size_t cap = std::max<size_t>(std::max<size_t>(need, 2 * o->cap), 1024);
  DevGuard g;
  float* nx = nullptr; double* nc = nullptr;
  int rc;
  if ((rc = g.alloc(&nx, 2 * cap * 3)) || (gicp && (rc = g.alloc(&nc, 2 * cap * 6)))) return rc;
  if (o->has_kf && o->kf_n > 0) {
    SSLAM_HIP_TRY(hipMemcpyAsync(nx + (size_t)o->kf_slot * cap * 3, o->d_xyz + (size_t)o->kf_slot * o->cap * 3, (size_t)o->kf_n * 3 * sizeof(float),
                                 hipMemcpyDeviceToDevice, s->stream));
    if (gicp) SSLAM_HIP_TRY(hipMemcpyAsync(nc + (size_t)o->kf_slot * cap * 6, o->d_cov + (size_t)o->kf_slot * o->cap * 6, (size_t)o->kf_n * 6 * sizeof(double),
                                           hipMemcpyDeviceToDevice, s->stream));
    SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  }
  if (o->d_xyz) (void)hipFree(o->d_xyz);
  if (o->d_cov) (void)hipFree(o->d_cov);
  o->d_xyz = nx; o->d_cov = nc; o->cap = cap;
  g.ptrs.clear();                        // the handle owns them now
  return 0;
}
extern "C" {
void sslam_odom_default_params(sslam_odom_params* p) {
  if (!p) return;
  memset(p, 0, sizeof *p);
  sslam_prefilter_default_params(&p->prefilter);
  p->method = SSLAM_REG_GICP;            // hdl's default is FAST_GICP
  sslam_gicp_default_params(&p->gicp);
  p->max_iterations = 64; p->epsilon = 0.01; p->max_correspondence_distance = 2.5;
  p->keyframe_delta_trans = 0.25; p->keyframe_delta_angle = 0.15; p->keyframe_delta_time = 1.0;
  p->transform_thresholding = 0; p->max_acceptable_trans = 1.0; p->max_acceptable_angle = 1.0;
}
sslam_odom* sslam_odom_create(sslam_seg* seg, const sslam_odom_params* p) {
  if (!seg) { set_error(SSLAM_ERR_INVALID, "bad argument"); return nullptr; }
  sslam_odom_params P;
  if (p) P = *p; else sslam_odom_default_params(&P);
  if (odom_check_params(&P)) return nullptr;
  sslam_odom* o = new sslam_odom();
  o->seg = seg; o->P = P;
  odom_identity(o->kf_pose); odom_identity(o->prev);
  return o;
}
void sslam_odom_destroy(sslam_odom* o) { delete o; }
int sslam_odom_reset(sslam_odom* o) {
  if (!o) return set_error(SSLAM_ERR_INVALID, "bad argument");
  o->has_kf = false; o->kf_n = 0; o->keyframes = 0; o->cov_passes = 0; o->kf_sec = o->kf_nsec = 0;
  odom_identity(o->kf_pose); odom_identity(o->prev);
  return 0;
}
int sslam_odom_push(sslam_odom* o, const float* xyz, int n, int32_t stamp_sec, int32_t stamp_nsec, double pose_out[12], sslam_odom_stats* stats) {
  const auto t_start = std::chrono::steady_clock::now();
  if (!o || !xyz || !pose_out || n < 0) return set_error(SSLAM_ERR_INVALID, "bad argument");
  sslam_seg* s = o->seg;
  const sslam_odom_params& P = o->P;
  int rc = odom_check_params(&P);
  if (rc) return rc;
  if (s->q_busy || s->n_inflight > 0) return set_error(SSLAM_ERR_INVALID, "a batch is in flight: collect it first");
  if ((rc = seg_device(s))) return rc;
  const bool gicp = P.method == SSLAM_REG_GICP;
  if (!o->ev[0]) { SSLAM_HIP_TRY(hipEventCreate(&o->ev[0])); SSLAM_HIP_TRY(hipEventCreate(&o->ev[1])); }
  if (!s->f_e0) { SSLAM_HIP_TRY(hipEventCreate(&s->f_e0)); SSLAM_HIP_TRY(hipEventCreate(&s->f_e1)); }
  sslam_odom_stats st;
  memset(&st, 0, sizeof st);
  st.n_raw = n;
  // 1. the frame goes up once; the chain; its result into the frame's slot of the arena; its covariances
  DevGuard g;
  float* d_in = nullptr;
  const float* d_res = nullptr;
  int m = 0;
  int32_t cnt[3] = {0, 0, 0};
  if ((rc = g.alloc(&d_in, (size_t)n * 3))) return rc;
  if (n > 0) SSLAM_HIP_TRY(hipMemcpyAsync(d_in, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  SSLAM_HIP_TRY(hipEventRecord(o->ev[0], s->stream));
  if (n > 0 && (rc = prefilter_device(s, g, d_in, n, &P.prefilter, &d_res, &m, cnt))) return rc;
  SSLAM_HIP_TRY(hipEventRecord(o->ev[1], s->stream));
  st.n_filtered = m;
  if (!o->has_kf && m == 0) {
    SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
    return set_error(SSLAM_ERR_NUMERIC, "odometry: the first frame is empty after the prefilter (%d raw points): no keyframe", n);
  }
  if ((rc = odom_reserve(o, (size_t)m))) return rc;
  const int fs = o->has_kf ? 1 - o->kf_slot : 0;
  const size_t f0 = (size_t)fs * o->cap;
  if (m > 0) SSLAM_HIP_TRY(hipMemcpyAsync(o->d_xyz + f0 * 3, d_res, (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToDevice, s->stream));
  int64_t cov_passes = o->cov_passes;
  if (gicp && m > 0) {
    const int32_t one[2] = {(int32_t)f0, (int32_t)(f0 + m)};
    if ((rc = knn_cov_launch(s, g, o->d_xyz, one, 1, nullptr, P.gicp.k, P.gicp.plane_epsilon, o->d_cov, nullptr, true))) return rc;
    float ms = 0.0f;
    SSLAM_HIP_TRY(hipEventElapsedTime(&ms, s->f_e0, s->f_e1));
    st.covariance_ms = (double)ms;
    ++cov_passes;
  } else {
    SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  }
  {
    float ms = 0.0f;
    SSLAM_HIP_TRY(hipEventElapsedTime(&ms, o->ev[0], o->ev[1]));
    st.prefilter_ms = (double)ms;
  }
  double pose[12], T[12];
  bool promote = false;
  if (!o->has_kf) {                      // 2. the first keyframe
    odom_identity(pose); odom_identity(T);
    st.accepted = 1;
    promote = true;
  } else {                               // 3. the match: one pair of register_pairs over the arena
    const int n_slot[2] = {fs == 0 ? m : o->kf_n, fs == 1 ? m : o->kf_n};
    const int32_t starts[4] = {0, n_slot[0], (int32_t)o->cap, (int32_t)o->cap + n_slot[1]};   // clouds 0 and 2 are the slots, 1 is the gap
    sslam_reg_pair pr;
    pr.target = 2 * o->kf_slot; pr.source = 2 * fs;
    for (int k = 0; k < 12; ++k) pr.T0[k] = o->prev[k];
    pr.max_corr2 = P.max_correspondence_distance * P.max_correspondence_distance;
    sslam_reg_result res;
    memset(&res, 0, sizeof res);
    if ((rc = register_pairs(s, nullptr, starts, 3, &pr, 1, nullptr, gicp ? &P.gicp : nullptr, P.max_iterations, P.epsilon, &res, nullptr, nullptr,
                             &st.registration_ms, o->d_xyz, gicp ? o->d_cov : nullptr)) < 0) return rc;
    st.matched = 1; st.iterations = res.iterations; st.converged = res.converged; st.status = res.status; st.used = res.used; st.fitness = res.score;
    bool ok = res.status == 0;           // 4. hdl's hasConverged
    if (ok && P.transform_thresholding) {   // 5.
      double inv[12], delta[12];
      odom_inverse(o->prev, inv);
      odom_mul(inv, res.T, delta);
      if (odom_trans(delta) > P.max_acceptable_trans || odom_angle(delta) > P.max_acceptable_angle) ok = false;
    }
    if (!ok) {
      for (int k = 0; k < 12; ++k) T[k] = o->prev[k];
      odom_mul(o->kf_pose, o->prev, pose);
    } else {                             // 6.
      for (int k = 0; k < 12; ++k) T[k] = res.T[k];
      odom_mul(o->kf_pose, T, pose);
      st.accepted = 1;
      st.delta_trans = odom_trans(T);
      st.delta_angle = odom_angle(T);
      st.delta_time = ((double)stamp_sec - (double)o->kf_sec) + 1e-9 * ((double)stamp_nsec - (double)o->kf_nsec);
      promote = st.delta_trans > P.keyframe_delta_trans || st.delta_angle > P.keyframe_delta_angle || st.delta_time > P.keyframe_delta_time;   // 7.
    }
  }
  // nothing can fail from here on: the state changes
  o->cov_passes = cov_passes;
  if (st.accepted) for (int k = 0; k < 12; ++k) o->prev[k] = T[k];
  if (promote) {
    o->has_kf = true; o->kf_slot = fs; o->kf_n = m;
    for (int k = 0; k < 12; ++k) o->kf_pose[k] = pose[k];
    o->kf_sec = stamp_sec; o->kf_nsec = stamp_nsec;
    odom_identity(o->prev);
    ++o->keyframes;
    st.new_keyframe = 1;
  }
  st.keyframes = o->keyframes;
  st.covariance_passes = o->cov_passes;
  for (int k = 0; k < 12; ++k) { pose_out[k] = pose[k]; st.T[k] = T[k]; }
  st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
  if (stats) *stats = st;
  return 0;
}
int sslam_odom_keyframe(const sslam_odom* o, float* xyz_out, int max_out, double pose_out[12]) {
  if (!o || max_out < 0 || (!xyz_out && max_out > 0)) return set_error(SSLAM_ERR_INVALID, "bad argument");
  if (!o->has_kf) return 0;
  if (pose_out) for (int k = 0; k < 12; ++k) pose_out[k] = o->kf_pose[k];
  const int w = std::min(o->kf_n, max_out);
  if (w > 0) {
    SSLAM_HIP_TRY(hipSetDevice(seg_device_index(o->seg)));
    SSLAM_HIP_TRY(hipMemcpy(xyz_out, o->d_xyz + (size_t)o->kf_slot * o->cap * 3, (size_t)w * 3 * sizeof(float), hipMemcpyDeviceToHost));
  }
  return o->kf_n;
}

void sslam_inf_default_params(sslam_inf_params* p) {
  if (!p) return;
  // hdl_graph_slam's InformationMatrixCalculator defaults [UPSTREAM, unverified here]
  p->var_gain_a = 20.0; p->min_stddev_x = 0.1; p->max_stddev_x = 5.0; p->min_stddev_q = 0.05; p->max_stddev_q = 0.2; p->fitness_score_thresh = 0.5;
}

// InformationMatrixCalculator::weight (information_matrix_calculator.hpp:20-24)
static double fitness_weight(double a, double max_x, double min_y, double max_y, double x) {
  const double y = (1.0 - std::exp(-a * x)) / (1.0 - std::exp(-a * max_x));
  return min_y + (max_y - min_y) * y;
}

int sslam_information_from_fitness(const sslam_inf_params* p, double fitness, double info[36]) {
  if (!p || !info) return set_error(SSLAM_ERR_INVALID, "null argument");
  // information_matrix_calculator.cpp:39-50; the variances are the squares of the standard deviations
  const double min_var_x = p->min_stddev_x * p->min_stddev_x, max_var_x = p->max_stddev_x * p->max_stddev_x;
  const double min_var_q = p->min_stddev_q * p->min_stddev_q, max_var_q = p->max_stddev_q * p->max_stddev_q;
  const float w_x = (float)fitness_weight(p->var_gain_a, p->fitness_score_thresh, min_var_x, max_var_x, fitness);
  const float w_q = (float)fitness_weight(p->var_gain_a, p->fitness_score_thresh, min_var_q, max_var_q, fitness);
  std::memset(info, 0, 36 * sizeof(double));
  for (int k = 0; k < 3; ++k) { info[k * 7] = 1.0 / (double)w_x; info[(k + 3) * 7] = 1.0 / (double)w_q; }
  return 0;
}

}  // extern "C"
