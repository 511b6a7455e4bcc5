// scratch.h -- how scratch memory is laid out and who owns it.  A layout is stated ONCE, as a function that takes its pieces
// from a Carve in order; on a Carve without memory the same function measures the layout, so the byte count and the pointers
// cannot drift apart.  No HIP header is needed here: the struct compiles with any host compiler.
#pragma once
#include <stddef.h>

struct wass_ctx;

namespace wass {

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Hands `mem` out in 256-aligned pieces in the order asked and owns nothing.  With mem == nullptr take() hands out nullptr and
// still counts: `used` is then the layout's size.  A piece of 0 bytes takes no room and is a pointer nobody may follow.
struct Carve {
    char* mem = nullptr;
    size_t used = 0;
    template <class T> T* take(size_t bytes)
    {
        T* p = mem ? (T*)(mem + used) : nullptr;
        used += align256(bytes);
        return p;
    }
};

template <class F> size_t measure(F lay) { Carve a; lay(a); return a.used; }   // the size of the layout that lay(Carve&) states

// Device memory of the context's pool (or of a handle): grown by ensure(), never shrunk, freed with its owner, who has selected
// the device and synchronised.  ensure: at least `bytes` in b, in steps of 1 MiB; the contents do not survive growth (api.hip).
struct Buf {
    void* p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf();
};
int ensure(wass_ctx* c, Buf& b, size_t bytes);

// Measure, ensure, carve: afterwards b holds the layout of lay(Carve&) and lay has run on b's memory as it is NOW (ensure may
// have moved it), so whatever pointers lay fills are good.
template <class F> int carve_buf(wass_ctx* c, Buf& b, F lay)
{
    if (int rc = ensure(c, b, measure(lay))) return rc;
    Carve a{ (char*)b.p };
    lay(a);
    return 0;
}

}  // namespace wass
