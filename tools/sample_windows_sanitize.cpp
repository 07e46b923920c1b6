// Stand-alone check of the shared sample -> window rule under UBSan + ASan: fd_sample_windows (host only, no device) on samples at
// INT32_MIN / INT32_MAX with widths that select no layer and widths that select one, plus a few ordinary ones.  Exit 0: the call
// returned FD_OK, no extreme sample got a window, the four ordinary ones that have a window got it, and no sanitizer report.
// Build and run from the repository root (the library's host code is compiled with the sanitizers, its device code as usual):
//   mkdir -p build/san
//   for f in featuredetection_amd/csrc/*.hip featuredetection_amd/csrc/hostalgo.cpp; do
//     /opt/rocm/bin/hipcc -O1 -g -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=undefined,address \
//       -Xarch_host -fno-sanitize-recover=undefined -x hip -c $f -o build/san/$(basename ${f%.*}).o; done
//   /opt/rocm/lib/llvm/bin/clang++ -O1 -g -std=c++17 -Iinclude -fsanitize=undefined,address -fno-sanitize-recover=undefined \
//     -c tools/sample_windows_sanitize.cpp -o build/san/main.obj
//   /opt/rocm/bin/hipcc --offload-arch=gfx950 -fsanitize=undefined,address build/san/main.obj build/san/*.o -o build/san/sample_windows -ldl
//   build/san/sample_windows
#include <climits>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "fd_hip.h"
int main() {
    const int32_t index[3] = {1, 2, 3}, lw[3] = {76, 60, 48}, lh[3] = {57, 45, 36};
    const double scale[3] = {0.7937005259840998, 0.6299605249474367, 0.5};
    const int32_t ext[3] = {INT32_MIN, INT32_MAX, INT32_MAX - 1}, widths[7] = {1, 2, INT32_MAX, 25, 32, 40, INT32_MIN};
    std::vector<int32_t> s;
    for (int32_t v : ext)
        for (int32_t w : widths)
            for (int k = 0; k < 3; ++k) {
                const int32_t q[4] = {k == 2 ? 48 : v, k == 1 ? 36 : v, w, k == 0 ? w : v};
                s.insert(s.end(), q, q + 4);
            }
    const int32_t regular[][4] = {{48, 36, 0, 10}, {48, 36, -5, -5}, {48, 36, 40, 40}, {17, 36, 40, 40}, {19, 36, 40, 40}, {77, 36, 40, 40}, {79, 36, 40, 40}, {48, 36, 25, 25}};
    for (auto& q : regular) s.insert(s.end(), q, q + 4);
    const int n = (int)(s.size() / 4);
    std::vector<int32_t> out((size_t)4 * n, 7);
    const int rc = fd_sample_windows(3, index, scale, lw, lh, 0.7937005259840998, 20, 20, n, s.data(), out.data());
    int valid = 0, validExtreme = 0;
    for (int i = 0; i < n; ++i) { valid += out[4 * i + 3]; if (i < n - 8) validExtreme += out[4 * i + 3]; }
    std::printf("rc %d, %d samples, %d valid, %d extreme samples valid\n", rc, n, valid, validExtreme);
    return rc == 0 && validExtreme == 0 && valid == 4 ? 0 : 1;
}
