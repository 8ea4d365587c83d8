// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.
//
// Stand-in for what TextSLAM's cost-functor headers use of Ceres: the names of the cost-function wrappers (empty: nothing is
// solved here, oracle/ref_driver.cpp calls the functors' operator() itself) and Jet<T, N>, a value with N partial derivatives,
// on which the templated functors yield their ambient Jacobians the way automatic differentiation does.  Written from scratch.
#ifndef TSREF_SHIM_CERES
#define TSREF_SHIM_CERES
#include <cassert>
#include <cmath>
#include <vector>
#include "Eigen/Core"

namespace ceres {

// the scalar functions rotation.h calls unqualified inside this namespace, next to the Jet overloads below
using std::sqrt; using std::sin; using std::cos; using std::acos; using std::asin; using std::atan2; using std::abs; using std::fabs;

class CostFunction {
public:
    virtual ~CostFunction() {}
};
template <typename Functor, int... Sizes> class AutoDiffCostFunction : public CostFunction {
public:
    explicit AutoDiffCostFunction(Functor *f) : functor_(f) {}
    virtual ~AutoDiffCostFunction() { delete functor_; }
private:
    Functor *functor_;
};
enum NumericDiffMethodType { CENTRAL, FORWARD, RIDDERS };
template <typename Functor, NumericDiffMethodType Method, int... Sizes> class NumericDiffCostFunction : public CostFunction {
public:
    explicit NumericDiffCostFunction(Functor *f) : functor_(f) {}
    virtual ~NumericDiffCostFunction() { delete functor_; }
private:
    Functor *functor_;
};

template <typename T, int N> struct Jet {
    T a;            // value
    T v[N];         // partial derivatives
    Jet() : a(T(0)) { for (int i = 0; i < N; i++) v[i] = T(0); }
    Jet(const T &value) : a(value) { for (int i = 0; i < N; i++) v[i] = T(0); }      // a constant
    Jet(const T &value, int k) : a(value) { for (int i = 0; i < N; i++) v[i] = T(0); v[k] = T(1); }   // the k-th variable
};
template <typename T, int N> Jet<T, N> operator+(const Jet<T, N> &f, const Jet<T, N> &g) { Jet<T, N> h; h.a = f.a + g.a; for (int i = 0; i < N; i++) h.v[i] = f.v[i] + g.v[i]; return h; }
template <typename T, int N> Jet<T, N> operator-(const Jet<T, N> &f, const Jet<T, N> &g) { Jet<T, N> h; h.a = f.a - g.a; for (int i = 0; i < N; i++) h.v[i] = f.v[i] - g.v[i]; return h; }
template <typename T, int N> Jet<T, N> operator-(const Jet<T, N> &f) { Jet<T, N> h; h.a = -f.a; for (int i = 0; i < N; i++) h.v[i] = -f.v[i]; return h; }
template <typename T, int N> Jet<T, N> operator*(const Jet<T, N> &f, const Jet<T, N> &g) { Jet<T, N> h; h.a = f.a*g.a; for (int i = 0; i < N; i++) h.v[i] = f.a*g.v[i] + f.v[i]*g.a; return h; }
template <typename T, int N> Jet<T, N> operator/(const Jet<T, N> &f, const Jet<T, N> &g) {       // (f / g)' = (f' - (f / g) g') / g
    Jet<T, N> h; const T inv = T(1)/g.a; h.a = f.a*inv; for (int i = 0; i < N; i++) h.v[i] = (f.v[i] - h.a*g.v[i])*inv; return h;
}
template <typename T, int N> Jet<T, N> operator+(const Jet<T, N> &f, const T &s) { Jet<T, N> h = f; h.a = f.a + s; return h; }
template <typename T, int N> Jet<T, N> operator+(const T &s, const Jet<T, N> &f) { Jet<T, N> h = f; h.a = s + f.a; return h; }
template <typename T, int N> Jet<T, N> operator-(const Jet<T, N> &f, const T &s) { Jet<T, N> h = f; h.a = f.a - s; return h; }
template <typename T, int N> Jet<T, N> operator-(const T &s, const Jet<T, N> &f) { Jet<T, N> h = -f; h.a = s - f.a; return h; }
template <typename T, int N> Jet<T, N> operator*(const Jet<T, N> &f, const T &s) { Jet<T, N> h; h.a = f.a*s; for (int i = 0; i < N; i++) h.v[i] = f.v[i]*s; return h; }
template <typename T, int N> Jet<T, N> operator*(const T &s, const Jet<T, N> &f) { Jet<T, N> h; h.a = s*f.a; for (int i = 0; i < N; i++) h.v[i] = s*f.v[i]; return h; }
template <typename T, int N> Jet<T, N> operator/(const Jet<T, N> &f, const T &s) { Jet<T, N> h; const T inv = T(1)/s; h.a = f.a*inv; for (int i = 0; i < N; i++) h.v[i] = f.v[i]*inv; return h; }
template <typename T, int N> Jet<T, N> operator/(const T &s, const Jet<T, N> &g) { return Jet<T, N>(s)/g; }
template <typename T, int N> Jet<T, N> &operator+=(Jet<T, N> &f, const Jet<T, N> &g) { f = f + g; return f; }
template <typename T, int N> Jet<T, N> &operator-=(Jet<T, N> &f, const Jet<T, N> &g) { f = f - g; return f; }
template <typename T, int N> Jet<T, N> &operator*=(Jet<T, N> &f, const Jet<T, N> &g) { f = f*g; return f; }
template <typename T, int N> Jet<T, N> &operator/=(Jet<T, N> &f, const Jet<T, N> &g) { f = f/g; return f; }
template <typename T, int N> Jet<T, N> sqrt(const Jet<T, N> &f) { Jet<T, N> h; h.a = std::sqrt(f.a); const T k = T(1)/(T(2)*h.a); for (int i = 0; i < N; i++) h.v[i] = f.v[i]*k; return h; }
// comparisons look at the value only
template <typename T, int N> bool operator<(const Jet<T, N> &f, const Jet<T, N> &g) { return f.a < g.a; }
template <typename T, int N> bool operator>(const Jet<T, N> &f, const Jet<T, N> &g) { return f.a > g.a; }
template <typename T, int N> bool operator<=(const Jet<T, N> &f, const Jet<T, N> &g) { return f.a <= g.a; }
template <typename T, int N> bool operator>=(const Jet<T, N> &f, const Jet<T, N> &g) { return f.a >= g.a; }
template <typename T, int N> bool operator==(const Jet<T, N> &f, const Jet<T, N> &g) { return f.a == g.a; }
template <typename T, int N> bool operator!=(const Jet<T, N> &f, const Jet<T, N> &g) { return f.a != g.a; }

}  // namespace ceres
#endif
