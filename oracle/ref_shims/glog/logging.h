// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  Stand-in for the one glog macro rotation.h uses: the debug check is a no-op that
// still accepts a streamed message.
#ifndef TSREF_SHIM_GLOG
#define TSREF_SHIM_GLOG
namespace tsref_shim {
struct NullStream { template <typename T> NullStream &operator<<(const T &) { return *this; } };
}
#define DCHECK_NE(a, b) while (false) ::tsref_shim::NullStream()
#endif
