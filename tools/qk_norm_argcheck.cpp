// Host-side exercise of the argument checks of ucfvit_qk_norm_fwd / ucfvit_qk_norm_bwd / ucfvit_qk_norm_partial_rows (csrc/qk_norm.hip):
// every call below is refused (or returns at once for an empty input) before any HIP call, so the program needs no GPU.  Meant for a
// sanitizer build of the host code, on a machine without a device:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude \
//         ucf-vit_amd/csrc/qk_norm.hip ucf-vit_amd/csrc/api.hip tools/qk_norm_argcheck.cpp -o qk_norm_argcheck && ./qk_norm_argcheck
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

static void expect_rows(int64_t got, bool positive, const char* what) {
    if ((got > 0) != positive) {
        ++failures;
        std::printf("FAIL %s: partial rows %lld\n", what, (long long)got);
    }
}

int main() {
    alignas(16) static float buf[256] = {0};
    void* p = buf;
    void* odd = (char*)buf + 4;
    float* f = buf;
    const float* g = buf;
    const int BAD = UCFVIT_ERR_INVALID_ARGUMENT, F32 = UCFVIT_F32;
    // forward
    expect(ucfvit_qk_norm_fwd(nullptr, g, g, g, g, p, f, f, 4, 2, 32, 1e-6f, F32, nullptr), BAD, "null pointer", "fwd: null qkv");
    expect(ucfvit_qk_norm_fwd(p, nullptr, g, g, g, p, f, f, 4, 2, 32, 1e-6f, F32, nullptr), BAD, "null parameter", "fwd: null gamma_q");
    expect(ucfvit_qk_norm_fwd(p, g, nullptr, g, g, p, f, f, 4, 2, 32, 1e-6f, F32, nullptr), BAD, "null parameter", "fwd: null beta_q");
    expect(ucfvit_qk_norm_fwd(p, g, g, nullptr, g, p, f, f, 4, 2, 32, 1e-6f, F32, nullptr), BAD, "null parameter", "fwd: null gamma_k");
    expect(ucfvit_qk_norm_fwd(p, g, g, g, nullptr, p, f, f, 4, 2, 32, 1e-6f, F32, nullptr), BAD, "null parameter", "fwd: null beta_k");
    expect(ucfvit_qk_norm_fwd(p, g, g, g, g, p, nullptr, nullptr, 4, 2, 32, 1e-6f, F32, nullptr), BAD, "go together", "fwd: saved without stats");
    expect(ucfvit_qk_norm_fwd(p, g, g, g, g, nullptr, f, f, 4, 2, 32, 1e-6f, F32, nullptr), BAD, "go together", "fwd: stats without saved");
    expect(ucfvit_qk_norm_fwd(p, g, g, g, g, p, f, nullptr, 4, 2, 32, 1e-6f, F32, nullptr), BAD, "go together", "fwd: mean without rstd");
    expect(ucfvit_qk_norm_fwd(p, g, g, g, g, p, f, f, 4, 2, 48, 1e-6f, F32, nullptr), BAD, "dh=48", "fwd: dh = 48");
    expect(ucfvit_qk_norm_fwd(p, g, g, g, g, p, f, f, 4, 2, 0, 1e-6f, F32, nullptr), BAD, "dh=0", "fwd: dh = 0");
    expect(ucfvit_qk_norm_fwd(p, g, g, g, g, p, f, f, 4, 2, 256, 1e-6f, F32, nullptr), BAD, "dh=256", "fwd: dh = 256");
    expect(ucfvit_qk_norm_fwd(p, g, g, g, g, p, f, f, 4, 0, 32, 1e-6f, F32, nullptr), BAD, "H=0", "fwd: H = 0");
    expect(ucfvit_qk_norm_fwd(p, g, g, g, g, p, f, f, 4, 1ll << 40, 32, 1e-6f, F32, nullptr), BAD, "bad head count", "fwd: H huge");
    expect(ucfvit_qk_norm_fwd(p, g, g, g, g, p, f, f, -1, 2, 32, 1e-6f, F32, nullptr), BAD, "bad row count -1", "fwd: rows < 0");
    expect(ucfvit_qk_norm_fwd(p, g, g, g, g, p, f, f, 1ll << 31, 2, 32, 1e-6f, F32, nullptr), BAD, "bad row count", "fwd: rows = 2^31");
    expect(ucfvit_qk_norm_fwd(p, g, g, g, g, p, f, f, 4, 2, 32, -1.f, F32, nullptr), BAD, "bad eps", "fwd: eps < 0");
    expect(ucfvit_qk_norm_fwd(p, g, g, g, g, p, f, f, 4, 2, 32, std::nanf(""), F32, nullptr), BAD, "bad eps", "fwd: eps NaN");
    expect(ucfvit_qk_norm_fwd(p, g, g, g, g, p, f, f, 4, 2, 32, 1e-6f, 7, nullptr), BAD, "dtype", "fwd: dtype");
    expect(ucfvit_qk_norm_fwd(odd, g, g, g, g, p, f, f, 4, 2, 32, 1e-6f, F32, nullptr), BAD, "16-byte aligned", "fwd: qkv alignment");
    expect(ucfvit_qk_norm_fwd(p, g, g, g, g, odd, f, f, 4, 2, 32, 1e-6f, F32, nullptr), BAD, "16-byte aligned", "fwd: saved alignment");
    expect(ucfvit_qk_norm_fwd(p, g, g, g, g, nullptr, nullptr, nullptr, 0, 2, 32, 0.f, UCFVIT_BF16, nullptr), UCFVIT_OK, "", "fwd: no rows");
    expect(ucfvit_qk_norm_fwd(p, g, g, g, g, p, f, f, 0, 16, 128, 1e-6f, F32, nullptr), UCFVIT_OK, "", "fwd: no rows, saving");
    // backward
    expect(ucfvit_qk_norm_bwd(nullptr, p, g, g, g, g, nullptr, nullptr, 4, 2, 32, F32, nullptr), BAD, "null pointer", "bwd: null dqkv");
    expect(ucfvit_qk_norm_bwd(p, nullptr, g, g, g, g, nullptr, nullptr, 4, 2, 32, F32, nullptr), BAD, "null pointer", "bwd: null saved");
    expect(ucfvit_qk_norm_bwd(p, p, g, g, nullptr, g, nullptr, nullptr, 4, 2, 32, F32, nullptr), BAD, "null pointer", "bwd: null mean");
    expect(ucfvit_qk_norm_bwd(p, p, g, g, g, nullptr, nullptr, nullptr, 4, 2, 32, F32, nullptr), BAD, "null pointer", "bwd: null rstd");
    expect(ucfvit_qk_norm_bwd(p, p, nullptr, g, g, g, nullptr, nullptr, 4, 2, 32, F32, nullptr), BAD, "null parameter", "bwd: null gamma_q");
    expect(ucfvit_qk_norm_bwd(p, p, g, nullptr, g, g, nullptr, nullptr, 4, 2, 32, F32, nullptr), BAD, "null parameter", "bwd: null gamma_k");
    expect(ucfvit_qk_norm_bwd(p, p, g, g, g, g, nullptr, nullptr, 4, 2, 96, F32, nullptr), BAD, "dh=96", "bwd: dh = 96");
    expect(ucfvit_qk_norm_bwd(p, p, g, g, g, g, nullptr, nullptr, 4, -2, 32, F32, nullptr), BAD, "H=-2", "bwd: H < 0");
    expect(ucfvit_qk_norm_bwd(p, p, g, g, g, g, nullptr, nullptr, -4, 2, 32, F32, nullptr), BAD, "bad row count -4", "bwd: rows < 0");
    expect(ucfvit_qk_norm_bwd(p, p, g, g, g, g, nullptr, nullptr, 4, 2, 32, -1, nullptr), BAD, "dtype", "bwd: dtype");
    expect(ucfvit_qk_norm_bwd(odd, p, g, g, g, g, nullptr, nullptr, 4, 2, 32, F32, nullptr), BAD, "16-byte aligned", "bwd: dqkv alignment");
    expect(ucfvit_qk_norm_bwd(p, odd, g, g, g, g, nullptr, nullptr, 4, 2, 32, F32, nullptr), BAD, "16-byte aligned", "bwd: saved alignment");
    expect(ucfvit_qk_norm_bwd(p, p, g, g, g, g, f, nullptr, 0, 2, 32, F32, nullptr), BAD, "empty input", "bwd: parameter sums of no rows");
    expect(ucfvit_qk_norm_bwd(p, p, g, g, g, g, nullptr, f, 0, 2, 32, F32, nullptr), BAD, "empty input", "bwd: column sums of no rows");
    expect(ucfvit_qk_norm_bwd(p, p, g, g, g, g, nullptr, nullptr, 0, 2, 32, F32, nullptr), UCFVIT_OK, "", "bwd: no rows");
    // the row count of the partials
    expect_rows(ucfvit_qk_norm_partial_rows(0, 2, 32), false, "partial rows: no rows");
    expect_rows(ucfvit_qk_norm_partial_rows(4, 0, 32), false, "partial rows: H = 0");
    expect_rows(ucfvit_qk_norm_partial_rows(4, 2, 40), false, "partial rows: dh = 40");
    expect_rows(ucfvit_qk_norm_partial_rows(1ll << 31, 2, 32), false, "partial rows: rows = 2^31");
    expect_rows(ucfvit_qk_norm_partial_rows(1, 1, 32), true, "partial rows: one row");
    expect_rows(ucfvit_qk_norm_partial_rows(665 * 197, 16, 64), true, "partial rows: the ViT-L stream");
    if (ucfvit_qk_norm_partial_rows(1, 1, 32) != 1 || ucfvit_qk_norm_partial_rows(665 * 197, 16, 64) > 1024) {
        ++failures;
        std::printf("FAIL partial rows: 1 row must give 1 chunk, no input more than 1024\n");
    }
    std::printf("%s (%d failures)\n", failures ? "FAILED" : "all argument checks behave", failures);
    return failures ? 1 : 0;
}
