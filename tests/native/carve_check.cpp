// carve_check.cpp -- wass::Carve (wass_amd/csrc/scratch.h) on the host: a Carve without memory measures what a Carve over a block
// hands out.  Exit status 0 and "ok", or the first failed check.
#include "../../wass_amd/csrc/scratch.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

int main()
{
    const size_t sizes[] = { 1, 0, 255, 256, 257, 0, 0, 7, 4096, 100000, 3 * 33 * 8, 0, 1 };
    const size_t n = sizeof sizes / sizeof sizes[0];
    const auto lay = [&](wass::Carve& a, char** piece) { for (size_t i = 0; i < n; ++i) piece[i] = a.take<char>(sizes[i]); };
    char* none[n];
    char* piece[n];
    wass::Carve null;
    lay(null, none);
    char* block = (char*)aligned_alloc(256, null.used);      // exactly what was measured: one byte more is out of bounds
    wass::Carve real{ block };
    lay(real, piece);
    if (real.used != null.used || wass::measure([&](wass::Carve& a) { lay(a, none); }) != null.used) return puts("used differs"), 1;
    for (size_t i = 0; i < n; ++i) {
        if (none[i]) return printf("piece %zu of a null Carve is not null\n", i), 1;
        if ((uintptr_t)piece[i] % 256) return printf("piece %zu is not 256-aligned\n", i), 1;
        if (i + 1 < n && piece[i] + sizes[i] > piece[i + 1]) return printf("piece %zu overlaps the next\n", i), 1;
        for (size_t k = 0; k < sizes[i]; ++k) piece[i][k] = (char)i;                     // every byte of every piece is the block's
    }
    if (piece[0] != block || piece[n - 1] + sizes[n - 1] > block + real.used) return puts("the last piece ends past used"), 1;
    for (size_t i = 0; i < n; ++i)
        for (size_t k = 0; k < sizes[i]; ++k)
            if (piece[i][k] != (char)i) return printf("piece %zu was written over\n", i), 1;
    free(block);
    return puts("ok"), 0;
}
