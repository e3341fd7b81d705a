// vtkm_min.h: the least of VTK-m that the reference's header-only path-tracing
// worklets need to compile and run on the host, written from VTK-m's published
// semantics.  TEST INFRASTRUCTURE ONLY (tests/cpp/ref_stage_driver.cpp); the
// product's include/vtkm_compat/ is separate and is not used here.
//
// Every behaviour restated here is an assumption about VTK-m and is listed in
// DESIGN.md section 2, "Oracle assumptions":
//   Dot sums left to right; Cross is the plain difference of products;
//   MagnitudeSquared = Dot(x,x); Magnitude = Sqrt of it; RMagnitude =
//   RSqrt of it with the CPU RSqrt(x) = 1/Sqrt(x); Normalize(x): x = x *
//   RMagnitude(x); TriangleNormal(a,b,c) = Cross(b-a, c-a);
//   Epsilon<Float32>() = 1e-5f; Pi() is Float64; Pi_180f() is the float
//   constant; Vec<T> op T is per component in T; Vec<T> op Float64 is per
//   component in double, narrowed to T; Min(x,y) = y < x ? y : x and
//   Max(x,y) = x < y ? y : x for integers, fmin/fmax for floats; a default
//   constructed Vec is uninitialised; Sum and Multiply are a + b and a * b,
//   per component on a Vec<Float32, 4>; Algorithm::CopyIf(input, stencil,
//   output, predicate) writes, in order, the input values whose stencil
//   value satisfies the predicate.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#define VTKM_EXEC
#define VTKM_CONT
#define VTKM_EXEC_CONT
#define VTKM_SUPPRESS_EXEC_WARNINGS
#define VTKM_IS_DEVICE_ADAPTER_TAG(tag) static_assert(true, "")

namespace vtkm {
using Id = long long;
using IdComponent = int;
using Int8 = std::int8_t;
using UInt8 = std::uint8_t;
using Int32 = std::int32_t;
using UInt32 = std::uint32_t;
using Float32 = float;
using Float64 = double;

template <typename T, IdComponent N>
class Vec {
public:
  Vec() = default;
  explicit Vec(const T& v) {
    for (IdComponent i = 0; i < N; ++i) c[i] = v;
  }
  template <typename... Ts, typename = typename std::enable_if<(sizeof...(Ts) == N) && (N > 1)>::type>
  Vec(const Ts&... vs) : c{static_cast<T>(vs)...} {}
  template <typename U>
  explicit Vec(const Vec<U, N>& o) {
    for (IdComponent i = 0; i < N; ++i) c[i] = static_cast<T>(o[i]);
  }
  T& operator[](IdComponent i) { return c[i]; }
  const T& operator[](IdComponent i) const { return c[i]; }
  T c[N];
};

#define VTKM_MIN_VECVEC(OP)                                              \
  template <typename T, IdComponent N>                                   \
  inline Vec<T, N> operator OP(const Vec<T, N>& a, const Vec<T, N>& b) { \
    Vec<T, N> r;                                                         \
    for (IdComponent i = 0; i < N; ++i) r[i] = a[i] OP b[i];             \
    return r;                                                            \
  }
VTKM_MIN_VECVEC(+)
VTKM_MIN_VECVEC(-)
VTKM_MIN_VECVEC(*)
VTKM_MIN_VECVEC(/)
#undef VTKM_MIN_VECVEC

template <typename T, IdComponent N>
inline Vec<T, N> operator-(const Vec<T, N>& a) {
  Vec<T, N> r;
  for (IdComponent i = 0; i < N; ++i) r[i] = -a[i];
  return r;
}

// Vec op scalar: the scalar of the Vec's own type, or a Float64 (computed in
// double and narrowed per component).  As in VTK-m, T is deduced from both
// arguments, so Vec<Float32> * Float64 selects the second form.
template <typename T, IdComponent N>
inline Vec<T, N> operator*(Vec<T, N> a, T s) {
  for (IdComponent i = 0; i < N; ++i) a[i] = a[i] * s;
  return a;
}
template <typename T, IdComponent N>
inline Vec<T, N> operator*(T s, Vec<T, N> a) {
  for (IdComponent i = 0; i < N; ++i) a[i] = s * a[i];
  return a;
}
template <typename T, IdComponent N>
inline Vec<T, N> operator/(Vec<T, N> a, T s) {
  for (IdComponent i = 0; i < N; ++i) a[i] = a[i] / s;
  return a;
}
template <typename T, IdComponent N, typename = typename std::enable_if<!std::is_same<T, Float64>::value>::type>
inline Vec<T, N> operator*(Vec<T, N> a, Float64 s) {
  for (IdComponent i = 0; i < N; ++i) a[i] = static_cast<T>(static_cast<Float64>(a[i]) * s);
  return a;
}
template <typename T, IdComponent N, typename = typename std::enable_if<!std::is_same<T, Float64>::value>::type>
inline Vec<T, N> operator*(Float64 s, Vec<T, N> a) {
  for (IdComponent i = 0; i < N; ++i) a[i] = static_cast<T>(s * static_cast<Float64>(a[i]));
  return a;
}
template <typename T, IdComponent N, typename = typename std::enable_if<!std::is_same<T, Float64>::value>::type>
inline Vec<T, N> operator/(Vec<T, N> a, Float64 s) {
  for (IdComponent i = 0; i < N; ++i) a[i] = static_cast<T>(static_cast<Float64>(a[i]) / s);
  return a;
}

// ---- vtkm/Math.h
inline Float64 Pi() { return 3.14159265358979323846264338327950288; }
inline Float32 Pi_180f() { return 0.01745329251994329577f; }
template <typename T>
inline T Epsilon();
template <>
inline Float32 Epsilon<Float32>() { return 1e-5f; }
template <>
inline Float64 Epsilon<Float64>() { return 1e-9; }
inline Float32 Abs(Float32 x) { return std::fabs(x); }
inline Float64 Abs(Float64 x) { return std::fabs(x); }
inline Float32 Sqrt(Float32 x) { return std::sqrt(x); }
inline Float64 Sqrt(Float64 x) { return std::sqrt(x); }
inline Float32 RSqrt(Float32 x) { return 1 / Sqrt(x); }
inline Float64 RSqrt(Float64 x) { return 1 / Sqrt(x); }
inline Float32 Min(Float32 x, Float32 y) { return std::fmin(x, y); }
inline Float32 Max(Float32 x, Float32 y) { return std::fmax(x, y); }
inline Float64 Min(Float64 x, Float64 y) { return std::fmin(x, y); }
inline Float64 Max(Float64 x, Float64 y) { return std::fmax(x, y); }
template <typename T>
inline T Min(const T& x, const T& y) { return (y < x) ? y : x; }
template <typename T>
inline T Max(const T& x, const T& y) { return (x < y) ? y : x; }

// ---- vtkm/VectorAnalysis.h
template <typename T>
inline T Dot(const Vec<T, 3>& a, const Vec<T, 3>& b) { return T((a[0] * b[0]) + (a[1] * b[1]) + (a[2] * b[2])); }
template <typename T>
inline T dot(const Vec<T, 3>& a, const Vec<T, 3>& b) { return Dot(a, b); }
template <typename T>
inline Vec<T, 3> Cross(const Vec<T, 3>& x, const Vec<T, 3>& y) {
  return Vec<T, 3>(x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]);
}
template <typename T>
inline T MagnitudeSquared(const Vec<T, 3>& x) { return Dot(x, x); }
template <typename T>
inline T Magnitude(const Vec<T, 3>& x) { return Sqrt(MagnitudeSquared(x)); }
template <typename T>
inline T RMagnitude(const Vec<T, 3>& x) { return RSqrt(MagnitudeSquared(x)); }
template <typename T>
inline Vec<T, 3> Normal(const Vec<T, 3>& x) { return x * RMagnitude(x); }
template <typename T>
inline void Normalize(Vec<T, 3>& x) { x = x * RMagnitude(x); }
template <typename T>
inline Vec<T, 3> TriangleNormal(const Vec<T, 3>& a, const Vec<T, 3>& b, const Vec<T, 3>& c) {
  return Cross(b - a, c - a);
}

// ---- vtkm/BinaryOperators.h
struct Sum {
  template <typename T, typename U>
  auto operator()(const T& a, const U& b) const -> decltype(a + b) { return a + b; }
};
struct Multiply {
  template <typename T, typename U>
  auto operator()(const T& a, const U& b) const -> decltype(a * b) { return a * b; }
};

// ---- vtkm/exec: names that PathAlgorithms.h mentions
namespace exec {
struct FunctorBase {};
namespace internal {
struct ErrorMessageBuffer {};
} // namespace internal
} // namespace exec

// ---- vtkm/cont: an ArrayHandle that only lends out plain pointer portals
namespace cont {
struct DeviceAdapterTagSerial {};
struct DeviceAdapterTagAny {};
struct DeviceAdapterId {};
struct StorageTagBasic {};
struct Token {};
struct ExecutionObjectBase {};
// Named by PathAlgorithms.h's host-side dispatch templates, which the stage driver never instantiates: it
// runs the kernel functors of that header itself.
template <typename Device>
struct DeviceAdapterAlgorithm;
namespace internal {
template <typename In, typename Out>
struct CopyKernel {
  CopyKernel(In, Out, Id) {}
};
} // namespace internal
namespace detail {
template <typename Device, typename T>
void PrepareArgForExec(T&&, Token&) {}
} // namespace detail
template <typename Functor, typename... Args>
void TryExecuteOnDevice(DeviceAdapterId, Functor&&, Args&&...) {}

template <typename T>
struct ArrayPortal {
  T* p = nullptr;
  Id n = 0;
  Id GetNumberOfValues() const { return n; }
  T Get(Id i) const { return p[i]; }
  void Set(Id i, const T& v) const { p[i] = v; }
};

template <typename T, typename Storage = StorageTagBasic>
class ArrayHandle {
public:
  template <typename Device>
  struct ExecutionTypes {
    using PortalConst = ArrayPortal<const T>;
    using Portal = ArrayPortal<T>;
  };
  ArrayHandle() = default;
  ArrayHandle(const T* p, Id n) : P(p), N(n) {}
  template <typename Device>
  ArrayPortal<const T> PrepareForInput(Device, Token&) const {
    ArrayPortal<const T> r;
    r.p = P;
    r.n = N;
    return r;
  }
  Id GetNumberOfValues() const { return N; }

private:
  const T* P = nullptr;
  Id N = 0;
};

// The implicit arrays and the one algorithm of MapperPathTracer.cxx:265-267.
template <typename T>
struct ArrayHandleCounting {
  T Start, Step;
  Id N;
  ArrayHandleCounting(T start, T step, Id n) : Start(start), Step(step), N(n) {}
  Id GetNumberOfValues() const { return N; }
  T Get(Id i) const { return static_cast<T>(Start + Step * static_cast<T>(i)); }
};
template <typename T>
struct ArrayHandleConstant {
  T Value;
  Id N;
  ArrayHandleConstant(T value, Id n) : Value(value), N(n) {}
  Id GetNumberOfValues() const { return N; }
  T Get(Id) const { return Value; }
};
struct Algorithm {
  // Stream compaction: output = the input values whose stencil value satisfies the predicate, in order.
  template <typename In, typename Stencil, typename T, typename Predicate>
  static void CopyIf(const In& input, const Stencil& stencil, std::vector<T>& output, Predicate predicate) {
    output.clear();
    for (Id i = 0; i < input.GetNumberOfValues(); ++i)
      if (predicate(stencil.Get(i))) output.push_back(input.Get(i));
  }
};
} // namespace cont

// ---- vtkm/worklet: the signature tags and nothing behind them
namespace worklet {
class WorkletMapField {
public:
  struct FieldIn {};
  struct FieldOut {};
  struct FieldInOut {};
  struct WholeArrayIn {};
  struct WholeArrayOut {};
  struct WholeArrayInOut {};
  struct ExecObject {};
  struct WorkIndex {};
  struct _1 {};
  struct _2 {};
  struct _3 {};
  struct _4 {};
  struct _5 {};
  struct _6 {};
  struct _7 {};
  struct _8 {};
  struct _9 {};
  struct _10 {};
  struct _11 {};
  struct _12 {};
  struct _13 {};
};
} // namespace worklet
} // namespace vtkm
