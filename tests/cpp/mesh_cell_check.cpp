// mesh_cell_check.cpp -- csrc/rtp_mesh_cell.hpp as plain host C++: the float
// helpers against the standard library, half_outward against the binary
// search over the halves' values that the host builder used before the two
// builders shared one rule, and the pads and boxes of hand-made cells against
// the formula of rtp_layout.hpp (kMeshCosMin) written out here.  No HIP, no
// library: build.build_mesh_cell_check(), and sanitized by build.build_asan().
// Prints "OK" and exits 0 when every check passes.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rtp_mesh_cell.hpp"

static int failures = 0;
#define EXPECT(cond)                                             \
  do {                                                           \
    if (!(cond) && failures++ < 20) std::fprintf(stderr, "FAIL %d: %s\n", __LINE__, #cond); \
  } while (0)

static uint32_t bits(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}
static float from_bits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

// the explicit values of the float checks, then a few thousand bit patterns (no NaN)
static std::vector<float> float_set() {
  std::vector<float> v = {0.f,      -0.f,     from_bits(1u), from_bits(0x80000001u), 1.f,       -1.f,
                          FLT_MAX,  -FLT_MAX, INFINITY,      -INFINITY,              FLT_MIN,   -FLT_MIN,
                          65504.f,  65505.f,  0x1p-24f,      1e-8f,                  -1e-8f,    0x1p100f};
  uint32_t s = 12345u;
  while (v.size() < 4096) {
    s = s * 1664525u + 1013904223u;
    const float f = from_bits(s ^ (s >> 15));
    if (!std::isnan(f)) v.push_back(f);
  }
  return v;
}

static void check_next(const std::vector<float>& v) {
  for (float x : v) {
    EXPECT(bits(rtp::next_up(x)) == bits(std::nextafter(x, INFINITY)));
    EXPECT(bits(rtp::next_down(x)) == bits(std::nextafter(x, -INFINITY)));
    EXPECT(rtp::finite_f(x) == (bool)std::isfinite(x));
    EXPECT(rtp::finite_d((double)x) == (bool)std::isfinite((double)x));
    EXPECT(bits(rtp::min_of(x, 0.5f)) == bits(std::min(x, 0.5f)) && bits(rtp::max_of(x, 0.5f)) == bits(std::max(x, 0.5f)));
  }
  EXPECT(bits(rtp::min_of(0.f, -0.f)) == bits(std::min(0.f, -0.f)) && bits(rtp::min_of(-0.f, 0.f)) == bits(std::min(-0.f, 0.f)));
  EXPECT(bits(rtp::max_of(0.f, -0.f)) == bits(std::max(0.f, -0.f)) && bits(rtp::max_of(-0.f, 0.f)) == bits(std::max(-0.f, 0.f)));
  EXPECT(!rtp::finite_f(NAN) && !rtp::finite_d((double)NAN) && !rtp::finite_d((double)INFINITY));
}

static void check_keys(const std::vector<float>& v) {
  for (float x : v) EXPECT(bits(rtp::mesh_key_float(rtp::mesh_float_key(x))) == bits(x));
  // the key order is the '<' order; of the two zeros, which '<' does not order, -0 comes first
  for (size_t i = 0; i < v.size(); i++) {
    const float x = v[i], y = v[(i * 7 + 3) % v.size()];
    const uint32_t kx = rtp::mesh_float_key(x), ky = rtp::mesh_float_key(y);
    if (x < y) EXPECT(kx < ky);
    if (y < x) EXPECT(ky < kx);
    if (x == y && bits(x) == bits(y)) EXPECT(kx == ky);
  }
  EXPECT(rtp::mesh_float_key(-0.f) < rtp::mesh_float_key(0.f));
  EXPECT(rtp::mesh_float_key(-INFINITY) < rtp::mesh_float_key(-FLT_MAX) && rtp::mesh_float_key(FLT_MAX) < rtp::mesh_float_key(INFINITY));
}

// ---- half precision rounded outward: the independent statement ----
// the ordered key of a half: key k >= 0 is the half with bits k, k < 0 its negative
static float half_value(int key) {
  const int b = key < 0 ? -key : key;
  const int e = b >> 10, m = b & 0x3ff;
  const float v = e == 0 ? std::ldexp((float)m, -24) : e == 31 ? INFINITY : std::ldexp((float)(m | 0x400), e - 25);
  return key < 0 ? -v : v;
}
static float half_bits_value(uint32_t h) { return half_value((h & 0x8000u) ? -(int)(h & 0x7fffu) : (int)(h & 0x7fffu)); }
// the smallest half >= x (up) or the largest <= x, by binary search over the halves' values
static uint32_t half_outward_search(float x, bool up) {
  if (std::isnan(x)) return up ? 0x7c00u : 0xfc00u;
  int lo = -0x7c00, hi = 0x7c00;  // -inf .. +inf
  if (up) {
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if (half_value(mid) >= x) hi = mid;
      else lo = mid + 1;
    }
  } else {
    while (lo < hi) {
      const int mid = lo + (hi - lo + 1) / 2;
      if (half_value(mid) <= x) lo = mid;
      else hi = mid - 1;
    }
  }
  return lo < 0 ? 0x8000u | (uint32_t)(-lo) : (uint32_t)lo;
}
static void check_half_at(float x) {
  for (int up = 0; up < 2; up++) {
    const uint32_t got = rtp::half_outward(x, up != 0), want = half_outward_search(x, up != 0);
    EXPECT(got <= 0xffffu);
    EXPECT(half_bits_value(got) == half_bits_value(want));         // the value, everywhere
    if ((want & 0x7fffu) != 0) EXPECT(got == want);                // the bits, wherever the result is no zero
    if (!std::isnan(x)) EXPECT(up ? half_bits_value(got) >= x : half_bits_value(got) <= x);
  }
}
static void check_half() {
  // every exponent, both signs, a stride through the mantissas that is odd and ends on the last one
  for (uint32_t e = 0; e < 256; e++)
    for (uint32_t m = 0; m < 0x800000u; m += 0x1001u)
      for (uint32_t s = 0; s < 2; s++) {
        if (e == 255 && m != 0) continue;  // NaN: below
        check_half_at(from_bits(s << 31 | e << 23 | m));
        check_half_at(from_bits(s << 31 | e << 23 | (0x7fffffu - m)));
      }
  // every seventh half, and the floats next to it on both sides
  for (int k = -0x7c00; k <= 0x7c00; k += 7) {
    const float h = half_value(k);
    check_half_at(h), check_half_at(std::nextafter(h, INFINITY)), check_half_at(std::nextafter(h, -INFINITY));
  }
  for (float x : {0.f, -0.f, 65504.f, 65505.f, -65504.f, -65505.f, 1e-8f, -1e-8f, 0x1p-24f, -0x1p-24f, 0x1p-25f, -0x1p-25f,
                  1 + 0x1p-11f, 0x1p100f, -0x1p100f, 0.1f, -0.1f, 3.4e38f, -3.4e38f, 1e-30f, 6.1e-5f, -6.1e-5f})
    check_half_at(x);
  EXPECT(rtp::half_outward(NAN, true) == 0x7c00u && rtp::half_outward(NAN, false) == 0xfc00u);
  EXPECT(rtp::half_outward(0x1p100f, true) == 0x7c00u && rtp::half_outward(0x1p100f, false) == 0x7bffu);
  EXPECT(rtp::half_outward(-0x1p100f, false) == 0xfc00u && rtp::half_outward(-0x1p100f, true) == 0xfbffu);
  EXPECT(rtp::half_outward(65504.f, true) == 0x7bffu && rtp::half_outward(65505.f, true) == 0x7c00u);
  EXPECT(rtp::half_outward(65505.f, false) == 0x7bffu);
  EXPECT(rtp::half_outward(0x1p-24f, true) == 0x0001u && rtp::half_outward(0x1p-24f, false) == 0x0001u);
  EXPECT(rtp::half_outward(1e-8f, true) == 0x0001u && rtp::half_outward(-1e-8f, false) == 0x8001u);
  // the one place the rule and the search differ: the sign of a zero result
  EXPECT((rtp::half_outward(1e-8f, false) & 0x7fffu) == 0 && (rtp::half_outward(-1e-8f, true) & 0x7fffu) == 0);
  EXPECT(rtp::half_outward(0.f, true) == 0x0000u && rtp::half_outward(0.f, false) == 0x0000u);
  EXPECT((rtp::half_outward(-0.f, true) & 0x7fffu) == 0 && (rtp::half_outward(-0.f, false) & 0x7fffu) == 0);
}

// ---- pads and boxes: rtp_layout.hpp's formula, from each cell's sine and h as its construction gives them ----
static const double kCosMin = 0x1p-8, kRound = 0x1p-18, kMinSine = 0x1p-10;
static const float kHuge = 0x1p100f;
static float formula_pad(double sine, double h, double reach, double amax) {
  const double pad = (kRound * reach / sine + h) / kCosMin + (1e-5 + 0x1p-16 * amax + 0x1p-18 * reach);
  return std::nextafter((float)pad, INFINITY);
}
// within one float step (the sine here is the construction's, the header's comes from cross products)
static bool near_float(float got, float want) {
  return got == want || got == std::nextafter(want, INFINITY) || got == std::nextafter(want, -INFINITY);
}
static void check_box(const rtp::MeshCellBox& c, const float mn[3], const float mx[3]) {
  for (int k = 0; k < 3; k++) {
    EXPECT(bits(c.lo[k]) == bits(std::nextafter(mn[k] - c.pad, -INFINITY)));
    EXPECT(bits(c.hi[k]) == bits(std::nextafter(mx[k] + c.pad, INFINITY)));
    EXPECT(bits(c.cen[k]) == bits(0.5f * mn[k] + 0.5f * mx[k]));
  }
}
static void check_cells() {
  using rtp::d3;
  using rtp::f3;
  const float reach = 4.f;
  const float zero[3] = {0, 0, 0};
  {  // a unit square: sine 1, h 0, largest coordinate 1
    const f3 q{0, 0, 0}, r{1, 0, 0}, s{1, 1, 0}, t{0, 1, 0};
    const rtp::MeshCellBox c = rtp::mesh_cell_box(q, r, s, t, reach);
    const float mx[3] = {1, 1, 0};
    EXPECT(!c.tri && bits(c.pad) == bits(formula_pad(1.0, 0.0, reach, 1.0)));
    EXPECT(bits(c.pad) == bits(rtp::quad_pad(d3{0, 0, 0}, d3{1, 0, 0}, d3{1, 1, 0}, d3{0, 1, 0}, reach, 1.0)));
    EXPECT(c.pad > 0x1p-10f * reach && c.pad < 0x1p-9f * reach);
    check_box(c, zero, mx);
    const rtp::MeshCellRecord rec = rtp::mesh_cell_record(q, r, s, t, true);
    EXPECT(rec.para == 1 && rec.kind == 1 && rec.n.x == 0 && rec.n.y == 0 && rec.n.z == 1);
    EXPECT(rec.e01.x == 1 && rec.e03.y == 1 && rec.e21.y == -1 && rec.e23.x == -1);
  }
  {  // a triangle cell (a, b, c, c): sine 1 at v00; the box is the three vertices'
    const f3 q{0, 0, 0}, r{2, 0, 0}, t{0, 1, 0};
    const rtp::MeshCellBox c = rtp::mesh_cell_box(q, r, t, t, reach);
    const float mx[3] = {2, 1, 0};
    EXPECT(c.tri && bits(c.pad) == bits(formula_pad(1.0, 0.0, reach, 2.0)));
    EXPECT(bits(c.pad) == bits(rtp::tri_pad(d3{0, 0, 0}, d3{2, 0, 0}, d3{0, 1, 0}, reach, 2.0)));
    check_box(c, zero, mx);
    EXPECT(rtp::mesh_cell_record(q, r, t, t, true).kind == rtp::kMeshKindTri);
    EXPECT(rtp::mesh_cell_record(q, r, t, t, false).kind >= 0);
  }
  // slivers: a parallelogram and a triangle cell with the corner (1, 0, 0) ^ (1, y, 0), sine y / sqrt(1 + y^2)
  for (int above = 0; above < 2; above++) {
    const float y = above ? 0x1.4p-10f : 0x1.8p-11f;  // sine 1.25 and 0.75 of kMeshMinSine
    const double sine = (double)y / std::sqrt(1.0 + (double)y * y);
    EXPECT(above ? sine > kMinSine : sine < kMinSine);
    const f3 q{0, 0, 0}, r{1, 0, 0}, s{2, y, 0}, t{1, y, 0};
    const rtp::MeshCellBox cq = rtp::mesh_cell_box(q, r, s, t, reach), ct = rtp::mesh_cell_box(q, r, t, t, reach);
    if (above) {
      EXPECT(near_float(cq.pad, formula_pad(sine, 0.0, reach, 2.0)) && cq.pad < reach);
      EXPECT(near_float(ct.pad, formula_pad(sine, 0.0, reach, 1.0)) && ct.pad < reach);
    } else {
      EXPECT(cq.pad == kHuge && ct.pad == kHuge);
    }
    EXPECT(!cq.tri && ct.tri);
  }
  // bent quads: the unit square with v11 lifted by z; h = z, v11's projection w = sqrt(1/2) beyond the
  // diagonal, the second corner's sine sqrt(1 + 2 z^2) / (1 + z^2)
  for (int under = 0; under < 2; under++) {
    const float z = under ? 1.0e-3f : 1.8e-3f;
    const double h = z, w = std::sqrt(0.5), sine = std::sqrt(1 + 2 * h * h) / (1 + h * h);
    EXPECT(under ? h / w < kCosMin / 2 : h / w > kCosMin / 2);
    const rtp::MeshCellBox c = rtp::mesh_cell_box(f3{0, 0, 0}, f3{1, 0, 0}, f3{1, 1, z}, f3{0, 1, 0}, reach);
    if (under) {
      const float mx[3] = {1, 1, z};
      EXPECT(near_float(c.pad, formula_pad(sine, h, reach, 1.0)) && c.pad > 256 * z);
      check_box(c, zero, mx);
    } else {
      EXPECT(c.pad == kHuge);
    }
  }
  {  // a degenerate cell: four equal points
    const f3 p{0.25f, 0.5f, 0.75f};
    const rtp::MeshCellBox c = rtp::mesh_cell_box(p, p, p, p, reach);
    const float pp[3] = {p.x, p.y, p.z};
    EXPECT(c.tri && c.pad == kHuge);
    check_box(c, pp, pp);
    EXPECT(rtp::quad_pad(d3{1, 1, 1}, d3{1, 1, 1}, d3{1, 1, 1}, d3{1, 1, 1}, reach, 1.0) == kHuge);
  }
  {  // the reach: kBvhReachFactor diagonals
    const float lo[3] = {0, 0, 0}, hi[3] = {1, 2, 2};
    EXPECT(rtp::scene_reach(lo, hi) == 6.f);
  }
}

int main() {
  const std::vector<float> v = float_set();
  check_next(v);
  check_keys(v);
  check_half();
  check_cells();
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::puts("OK");
  return 0;
}
