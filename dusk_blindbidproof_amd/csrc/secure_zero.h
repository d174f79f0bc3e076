// Host memory: an erase the compiler cannot drop (the stores are volatile).  Secret wiping (include/bbp.h) uses it for every host copy
// of a secret before the memory is released; plain C++, no other header of the engine needed (submit.cpp, capi_prove.hip, the tests).
#pragma once
#include <stddef.h>

namespace bbp {

inline void secure_zero(void* p, size_t n) {
    volatile unsigned char* q = static_cast<volatile unsigned char*>(p);
    for (size_t i = 0; i < n; i++) q[i] = 0;
}
template <class V>
inline void secure_zero_vec(V& v) {  // the whole capacity: what a shrink left behind included
    const size_t n = v.size();
    v.resize(v.capacity());
    if (!v.empty()) secure_zero(v.data(), v.size() * sizeof(v[0]));
    v.resize(n);
}

}  // namespace bbp
