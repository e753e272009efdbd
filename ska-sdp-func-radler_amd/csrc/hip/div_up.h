// ceil(a / b), shared by the kernels' launchers (rdl_internal.h) and the
// host-only planning headers. Plain C++.
#pragma once
#include <cstddef>

namespace rdl {

inline unsigned DivUp(size_t a, size_t b) { return unsigned((a + b - 1) / b); }

}  // namespace rdl
