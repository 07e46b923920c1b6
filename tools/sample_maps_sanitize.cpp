// Stand-alone check of the wrapper-chain helpers under UBSan + ASan, host side only (no device is opened): fd_sample_maps_checked and
// fd_sample_maps_apply on zero maps, FD_SAMPLE_MAPS_MAX maps, one more than that, a kind the caller does not allow, a kind outside the
// mask's range and a NULL array with a positive count; fd_particle_sample against the two steps it is made of, on ordinary and extreme
// particles.  Exit 0: every case gave the code and the message part expected and no sanitizer reported.
// Build and run from the repository root (sample_windows_sanitize.cpp has the recipe for the whole library; this one needs hostalgo only):
//   mkdir -p build/san
//   S="-Xarch_host -fsanitize=undefined,address -Xarch_host -fno-sanitize-recover=undefined"
//   H="/opt/rocm/bin/hipcc -O1 -g -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Iinclude -Ifeaturedetection_amd/csrc $S -x hip -c"
//   $H featuredetection_amd/csrc/hostalgo.cpp -o build/san/hostalgo.o
//   $H tools/sample_maps_sanitize.cpp -o build/san/sample_maps_main.o
//   /opt/rocm/bin/hipcc --offload-arch=gfx950 -fsanitize=undefined,address build/san/sample_maps_main.o build/san/hostalgo.o -o build/san/sample_maps -ldl
//   build/san/sample_maps
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include "fd_internal.hpp"

static int failures = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { std::printf("FAILED: %s\n", what); ++failures; }
}

static const unsigned RESIZE = 1u << FD_SAMPLE_MAP_RESIZE, BOTH = RESIZE | 1u << FD_SAMPLE_MAP_INTEGRAL;

// the code of fd_sample_maps_checked and, where it throws, whether the message holds `part`; a chain that comes back is compared with its source
static int checked(const fd_sample_map* maps, int n, unsigned mask, const char* part) {
    try {
        const FdSampleMaps chain = fd_sample_maps_checked(maps, n, mask, "caller");
        expect(chain.n == n, "the count of the copy");
        for (int k = 0; k < n; ++k)
            expect(chain.m[k].kind == maps[k].kind && chain.m[k].factor == maps[k].factor && chain.m[k].x_offset == maps[k].x_offset &&
                       chain.m[k].y_offset == maps[k].y_offset, "a map of the copy");
        return FD_OK;
    } catch (const FdError& e) {
        expect(e.msg.find("caller: ") == 0 && e.msg.find(part) != std::string::npos, part);
        return e.code;
    }
}

int main() {
    fd_sample_map maps[FD_SAMPLE_MAPS_MAX + 1];
    for (int k = 0; k <= FD_SAMPLE_MAPS_MAX; ++k) maps[k] = fd_sample_map{FD_SAMPLE_MAP_RESIZE, 1.0 + 0.25 * k, 0.1 * k, -0.1 * k};
    int32_t s[8] = {48, 36, 25, 31, -7, 5, 40, 40}, before[8];
    std::memcpy(before, s, sizeof(s));

    expect(checked(nullptr, 0, BOTH, "") == FD_OK, "zero maps, NULL");
    expect(checked(maps, 0, RESIZE, "") == FD_OK, "zero maps");
    expect(checked(maps, FD_SAMPLE_MAPS_MAX, RESIZE, "") == FD_OK, "FD_SAMPLE_MAPS_MAX maps");
    expect(checked(maps, FD_SAMPLE_MAPS_MAX + 1, BOTH, "sample maps, at most") == FD_ERR_INVALID_ARGUMENT, "one map too many");
    expect(checked(nullptr, 2, BOTH, "bad argument") == FD_ERR_INVALID_ARGUMENT, "NULL with a positive count");
    expect(checked(maps, -1, BOTH, "bad argument") == FD_ERR_INVALID_ARGUMENT, "a negative count");
    maps[1].kind = FD_SAMPLE_MAP_INTEGRAL;
    expect(checked(maps, 3, BOTH, "") == FD_OK, "an integral map where it is allowed");
    expect(checked(maps, 3, RESIZE, "sample map kind 1; a pyramid chain takes FD_SAMPLE_MAP_RESIZE only") == FD_ERR_INVALID_ARGUMENT, "an integral map on a pyramid chain");
    const int32_t unknown[4] = {2, 32, -1, INT32_MIN};   // beside the kinds, past the mask's bits, negative
    for (int32_t kind : unknown) {
        maps[1].kind = kind;
        expect(checked(maps, 3, BOTH, "unknown sample map kind") == FD_ERR_INVALID_ARGUMENT, "an unknown kind");
        expect(fd_sample_maps_apply(maps, 3, 2, s) == FD_ERR_INVALID_ARGUMENT && std::memcmp(s, before, sizeof(s)) == 0, "apply: an unknown kind, samples untouched");
    }
    maps[1].kind = FD_SAMPLE_MAP_INTEGRAL;

    // fd_sample_maps_apply: the same rules as bare codes
    expect(fd_sample_maps_apply(nullptr, 0, 2, s) == FD_OK && std::memcmp(s, before, sizeof(s)) == 0, "apply: zero maps change nothing");
    expect(fd_sample_maps_apply(maps, FD_SAMPLE_MAPS_MAX + 1, 2, s) == FD_ERR_INVALID_ARGUMENT, "apply: one map too many");
    expect(fd_sample_maps_apply(nullptr, 1, 2, s) == FD_ERR_INVALID_ARGUMENT, "apply: NULL maps");
    expect(fd_sample_maps_apply(maps, 1, 2, nullptr) == FD_ERR_INVALID_ARGUMENT, "apply: NULL samples");
    expect(fd_sample_maps_apply(maps, 1, -1, s) == FD_ERR_INVALID_ARGUMENT, "apply: a negative sample count");
    expect(fd_sample_maps_apply(maps, FD_SAMPLE_MAPS_MAX, 2, s) == FD_OK, "apply: FD_SAMPLE_MAPS_MAX maps");

    // fd_particle_sample: the height rule, then the chain, on the host; extreme sizes and ratios saturate in fd_sample_cvround
    // (an integral map adds 1 to what it gets, which fd_hip.h expects below INT32_MAX: the extreme particles go through resize maps only)
    const FdSampleMaps mixed = fd_sample_maps_checked(maps, FD_SAMPLE_MAPS_MAX, BOTH, "caller");
    maps[1].kind = FD_SAMPLE_MAP_RESIZE;
    const FdSampleMaps resize = fd_sample_maps_checked(maps, FD_SAMPLE_MAPS_MAX, RESIZE, "caller");
    const FdSampleMaps none = fd_sample_maps_checked(nullptr, 0, BOTH, "caller");
    const int32_t values[7] = {0, 1, 25, -25, INT32_MAX, INT32_MIN, INT32_MAX - 1};
    const double aspects[5] = {1.0, 1.25, 0.0, 1e300, -3.5};
    for (const FdSampleMaps* m : {&none, &resize, &mixed})
        for (int32_t px : values)
            for (int32_t size : values)
                for (double aspect : aspects) {
                    if (m == &mixed && (px < -25 || px > 25 || size < -25 || size > 25 || aspect < 0.0 || aspect > 1.25)) continue;
                    const int32_t py = px / 2;
                    int32_t x, y, w, h;
                    fd_particle_sample(px, py, size, aspect, *m, x, y, w, h);
                    int32_t ex = px, ey = py, ew = size, eh = fd_sample_cvround(aspect * (double)size);
                    if (m->n == 0) expect(x == px && y == py && w == size && h == eh, "a particle without wrappers");
                    for (int k = 0; k < m->n; ++k) fd_sample_map_apply(m->m[k], ex, ey, ew, eh);
                    expect(x == ex && y == ey && w == ew && h == eh, "a particle through the chain");
                }
    std::printf("%d failures\n", failures);
    return failures == 0 ? 0 : 1;
}
