// Host-side exercise of the argument checks of ucfvit_layer_scale_add / ucfvit_layer_scale_grad (csrc/layer_scale.hip): every call below is
// refused (or returns at once for an empty input) before any HIP call, so the program needs no GPU.  Meant for a sanitizer build of the
// host code, on a machine without a device:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude \
//         ucf-vit_amd/csrc/layer_scale.hip ucf-vit_amd/csrc/api.hip tools/layer_scale_argcheck.cpp -o layer_scale_argcheck && ./layer_scale_argcheck
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "ucfvit_hip.h"

static int failures = 0;

static void expect(int rc, int want, const char* fragment, const char* what) {
    const char* err = ucfvit_last_error();
    const bool ok = rc == want && (want == UCFVIT_OK || (err && std::strstr(err, fragment)));
    if (!ok) {
        ++failures;
        std::printf("FAIL %s: rc=%d (want %d), error '%s' (want '%s')\n", what, rc, want, err ? err : "", fragment);
    }
}

int main() {
    float buf[64] = {0};
    void* p = buf;
    const float* g = buf;
    const int BAD = UCFVIT_ERR_INVALID_ARGUMENT, F32 = UCFVIT_F32;
    // forward
    expect(ucfvit_layer_scale_add(p, 8, nullptr, g, nullptr, p, 4, 8, 2, 1, 0.0, 0, F32, nullptr), BAD, "null pointer", "add: null branch");
    expect(ucfvit_layer_scale_add(p, 8, p, g, nullptr, nullptr, 4, 8, 2, 1, 0.0, 0, F32, nullptr), BAD, "null pointer", "add: null out");
    expect(ucfvit_layer_scale_add(p, 8, p, nullptr, nullptr, p, 4, 8, 2, 1, 0.0, 0, F32, nullptr), BAD, "null gamma", "add: null gamma");
    expect(ucfvit_layer_scale_add(p, 0, p, g, nullptr, p, 4, 0, 2, 1, 0.0, 0, F32, nullptr), BAD, "D=0", "add: D = 0");
    expect(ucfvit_layer_scale_add(p, 8, p, g, nullptr, p, 4, 8, 0, 1, 0.0, 0, F32, nullptr), BAD, "rows_per_sample=0", "add: rps = 0");
    expect(ucfvit_layer_scale_add(p, 8, p, g, nullptr, p, -4, 8, 2, 1, 0.0, 0, F32, nullptr), BAD, "bad row count", "add: rows < 0");
    expect(ucfvit_layer_scale_add(p, 8, p, g, nullptr, p, 1ll << 30, 8, 2, 1, 0.0, 0, F32, nullptr), BAD, "bad row count", "add: rows = 2^30");
    expect(ucfvit_layer_scale_add(p, 8, p, g, nullptr, p, 5, 8, 2, 1, 0.0, 0, F32, nullptr), BAD, "not a multiple", "add: rows % rps");
    expect(ucfvit_layer_scale_add(p, 7, p, g, nullptr, p, 4, 8, 2, 1, 0.0, 0, F32, nullptr), BAD, "ldr=7", "add: ldr < D");
    expect(ucfvit_layer_scale_add(p, 8, p, g, nullptr, p, 4, 8, 2, 1, 1.0, 0, F32, nullptr), BAD, "[0, 1)", "add: p = 1");
    expect(ucfvit_layer_scale_add(p, 8, p, g, nullptr, p, 4, 8, 2, 1, -0.5, 0, F32, nullptr), BAD, "[0, 1)", "add: p < 0");
    expect(ucfvit_layer_scale_add(p, 8, p, g, nullptr, p, 4, 8, 2, 1, std::nan(""), 0, F32, nullptr), BAD, "[0, 1)", "add: p = NaN");
    expect(ucfvit_layer_scale_add(p, 8, p, g, nullptr, p, 4, 8, 2, 0, 0.5, 0, F32, nullptr), BAD, "row_step=0", "add: row_step = 0");
    expect(ucfvit_layer_scale_add(p, 8, p, g, nullptr, p, 4, 8, 2, 1ll << 31, 0.5, 0, F32, nullptr), BAD, "row_step", "add: row_step huge");
    expect(ucfvit_layer_scale_add(p, 8, p, g, nullptr, p, 4, 8, 2, 1, 0.0, 0, 7, nullptr), BAD, "dtype", "add: dtype");
    expect(ucfvit_layer_scale_add(nullptr, 0, p, g, nullptr, p, 0, 8, 2, 1, 0.999999, ~0ull, F32, nullptr), UCFVIT_OK, "", "add: no rows");
    // backward
    expect(ucfvit_layer_scale_grad(nullptr, p, g, nullptr, p, nullptr, nullptr, 4, 8, 2, 1, 0.0, 0, F32, nullptr), BAD, "null pointer", "grad: dy");
    expect(ucfvit_layer_scale_grad(p, p, g, nullptr, nullptr, nullptr, nullptr, 4, 8, 2, 1, 0.0, 0, F32, nullptr), BAD, "null pointer", "grad: out");
    expect(ucfvit_layer_scale_grad(p, p, nullptr, nullptr, p, nullptr, nullptr, 4, 8, 2, 1, 0.0, 0, F32, nullptr), BAD, "null gamma", "grad: gamma");
    expect(ucfvit_layer_scale_grad(p, nullptr, g, nullptr, p, nullptr, buf, 4, 8, 2, 1, 0.0, 0, F32, nullptr), BAD, "branch is null",
           "grad: gamma sums without the branch");
    expect(ucfvit_layer_scale_grad(p, p, g, nullptr, p, nullptr, nullptr, 4, 0, 2, 1, 0.0, 0, F32, nullptr), BAD, "D=0", "grad: D = 0");
    expect(ucfvit_layer_scale_grad(p, p, g, nullptr, p, nullptr, nullptr, 4, 8, -1, 1, 0.0, 0, F32, nullptr), BAD, "rows_per_sample=-1", "grad: rps");
    expect(ucfvit_layer_scale_grad(p, p, g, nullptr, p, nullptr, nullptr, 7, 8, 2, 1, 0.0, 0, F32, nullptr), BAD, "not a multiple", "grad: rows % rps");
    expect(ucfvit_layer_scale_grad(p, p, g, nullptr, p, nullptr, nullptr, 4, 8, 2, 1, 1.5, 0, F32, nullptr), BAD, "[0, 1)", "grad: p > 1");
    expect(ucfvit_layer_scale_grad(p, p, g, nullptr, p, nullptr, nullptr, 4, 8, 2, -3, 0.5, 0, F32, nullptr), BAD, "row_step=-3", "grad: row_step");
    expect(ucfvit_layer_scale_grad(p, p, g, nullptr, p, nullptr, nullptr, 4, 8, 2, 1, 0.0, 0, -1, nullptr), BAD, "dtype", "grad: dtype");
    expect(ucfvit_layer_scale_grad(p, p, g, nullptr, p, buf, nullptr, 0, 8, 2, 1, 0.0, 0, F32, nullptr), BAD, "empty input", "grad: sums of no rows");
    expect(ucfvit_layer_scale_grad(p, nullptr, g, nullptr, p, nullptr, nullptr, 0, 8, 2, 1, 0.0, 0, F32, nullptr), UCFVIT_OK, "", "grad: no rows");
    std::printf("%s (%d failures)\n", failures ? "FAILED" : "all argument checks behave", failures);
    return failures ? 1 : 0;
}
