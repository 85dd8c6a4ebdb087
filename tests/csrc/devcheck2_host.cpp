// devcheck2_host.cpp -- TEST SHIM: the host build of the second operation table (devcheck_ops2.hpp), a loop over elements per
// operation.  tests/devcheck.py compares the gfx950 build of the same table (devcheck2.hip) with it bit for bit.  Not part of the product.
#include <stddef.h>
#include "devcheck_ops2.hpp"

extern "C" {
#define X(name, fn, IW, OW)                                                      \
  int dc_##name(const uint32_t* in, uint32_t* out, uint32_t n) {                 \
    for (uint32_t i = 0; i < n; i++) fn(in + (size_t)i * IW, out + (size_t)i * OW); \
    return 0;                                                                    \
  }
DC_OPS2(X)
#undef X
#define X(name, fn, IW, OW) #name ":" #IW ":" #OW ";"
const char* dc_table() { return DC_OPS2(X); }
#undef X
}
