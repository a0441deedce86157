// The layout of a handle's shell (limbo_amd/csrc/shell_layout.h) alone, on the host: built with -fsanitize=address,undefined and
// run by tests/test_shell_layout.py.  Every offset and size is pinned to the value the engine has always used (the header was
// written from literals spread over five files: nothing may have moved); then every region of the two blocks is written through
// the layout's accessors at its largest extent, in host buffers of exactly the two block sizes (AddressSanitizer is the witness
// that none leaves its block), and read back: no two regions share a byte.
#include "../../limbo_amd/csrc/shell_layout.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int fails = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            printf("FAIL " __VA_ARGS__); \
            printf("  [%s]\n", #cond);   \
            ++fails;                     \
        }                                \
    } while (0)

struct Region {
    const char* name;
    char* p;
    size_t bytes;
};

// every byte of every region gets the region's number, then is read back
static void fill_and_check(const Region* r, int n, const char* base, size_t block_bytes, const char* block)
{
    for (int i = 0; i < n; ++i) {
        const size_t off = (size_t)(r[i].p - base);
        CHECK(off <= block_bytes && r[i].bytes <= block_bytes - off, "%s block: %s [%zu, %zu) of %zu\n", block, r[i].name, off, off + r[i].bytes, block_bytes);
        memset(r[i].p, i + 1, r[i].bytes);
    }
    for (int i = 0; i < n; ++i)
        for (size_t k = 0; k < r[i].bytes; ++k)
            if (r[i].p[k] != i + 1) {
                CHECK(false, "%s block: byte %zu of %s was overwritten by region %d\n", block, k, r[i].name, r[i].p[k]);
                break;
            }
}

int main()
{
    using namespace shell;
    const size_t dbl = sizeof(double), tile = dbl * 4096;

    // ---- the numbers -------------------------------------------------------------------------------------------------
    CHECK(GPE_MAX_P == 8 && EDGE == 64 && PANEL == 256 && TILE == 4096, "tiles\n");
    CHECK(DEV_BYTES == 2170880 && HEAD_BYTES == 66 * tile && SCAL_DOUBLES == 1024 && HEAD_TILES == 66, "device block %zu\n", DEV_BYTES);
    CHECK(SCAL_LOGDET == 0 && SCAL_TRACE == 1 && SCAL_KNN == 2, "scalar slots\n");
    CHECK(HALF_TILES == 32 && STEP_HEAD_TILES == 6 && S22_TILE == 20 && S22_TILES == 9 && DIAG_SUM_TILE == 64 && FLAG_TILE == 65, "head block\n");
    CHECK(P256_POLLED_S == 9216 && P256_POLLED_DOUBLES == 33792, "polled buffer %d\n", (int)P256_POLLED_DOUBLES);
    CHECK(PINNED_BYTES == 18560 && INFO_BYTES == 64 && SEQ_OFF == 64 && SEQ_WORDS == 8 && HSCAL_OFF == 128 && HSCAL_DOUBLES == 1024
              && HSCAL_BYTES == 8192 && HSMALL_OFF == 128 + 8192,
          "pinned block %zu\n", PINNED_BYTES);
    CHECK(LL_PARTIALS == 8 && LL_MAX_BLOCKS == 256, "log-likelihood partials\n");
    CHECK(SMALL_DOUBLES == 1280 && SMALL_KTA == 16 && SMALL_VAR == 16 + 8 * GPE_MAX_P && SMALL_POINTS == 8 && SMALL_IN == 256
              && SMALL_IN_DOUBLES == 1024 && SMALL_MAX_N == 256 && SMALL_ADD_MAX_P == 3,
          "small path staging\n");

    // ---- the device block --------------------------------------------------------------------------------------------
    {
        char* base = (char*)malloc(DEV_BYTES); // exactly the block: one byte past it is AddressSanitizer's to report
        double* dev = (double*)base;
        CHECK((char*)head(dev) == base + 8192, "head block at 8 KiB\n");
        for (int par = 0; par < 2; ++par) {
            CHECK((char*)head_half(dev, par) == base + 8192 + par * 32 * tile, "half %d\n", par);
            CHECK((char*)s22(dev, par) == base + 8192 + (par * 32 + 20) * tile, "S22 of half %d\n", par);
            CHECK((char*)hflags(dev, par) == base + 8192 + 65 * tile + par * 32 * sizeof(flag_t), "flag words of half %d\n", par);
        }
        CHECK((char*)diag_sum(dev) == base + 8192 + 64 * tile && (char*)flag_tile(dev) == base + 8192 + 65 * tile, "the two single tiles\n");
        const Region r[] = {{"scalars", base, dbl * SCAL_DOUBLES},
                            {"head tiles 0", (char*)head_half(dev, 0), STEP_HEAD_TILES * tile},
                            {"S22 0", (char*)s22(dev, 0), S22_TILES * tile},
                            {"head tiles 1", (char*)head_half(dev, 1), STEP_HEAD_TILES * tile},
                            {"S22 1", (char*)s22(dev, 1), S22_TILES * tile},
                            {"diagonal sum", (char*)diag_sum(dev), tile},
                            {"flag words 0", (char*)hflags(dev, 0), HALF_TILES * sizeof(flag_t)},
                            {"flag words 1", (char*)hflags(dev, 1), HALF_TILES * sizeof(flag_t)}};
        fill_and_check(r, 8, base, DEV_BYTES, "device");
        memset(flag_tile(dev), 0, tile); // what gpe_create zeroes: the whole tile, the last of the block
        free(base);
    }

    // ---- the pinned block --------------------------------------------------------------------------------------------
    {
        char* base = (char*)malloc(PINNED_BYTES);
        CHECK((char*)info(base) == base && (char*)seq(base) == base + 64 && (char*)hscal(base) == base + 128, "info, sequence words, hScal\n");
        CHECK(ll_partials(base) == hscal(base) + 8 && small(base) == hscal(base) + 1024, "partials, hSmall\n");
        CHECK(small_kta(base) == small(base) + 16 && small_var(base) == small(base) + 16 + 8 * GPE_MAX_P && small_in(base) == small(base) + 256, "hSmall's slots\n");
        const Region r[] = {{"info words", (char*)info(base), INFO_BYTES},
                            {"sequence words", (char*)seq(base), SEQ_WORDS * sizeof(unsigned long long)},
                            {"log-likelihood terms", (char*)hscal(base), 2 * dbl},
                            {"partials", (char*)ll_partials(base), dbl * 2 * LL_MAX_BLOCKS},
                            {"small terms", (char*)small(base), 2 * dbl},
                            {"small kta", (char*)small_kta(base), dbl * SMALL_POINTS * GPE_MAX_P},
                            {"small var", (char*)small_var(base), dbl * SMALL_POINTS},
                            {"small inputs", (char*)small_in(base), dbl * SMALL_IN_DOUBLES}};
        fill_and_check(r, 8, base, PINNED_BYTES, "pinned");
        CHECK(small_in(base) + SMALL_IN_DOUBLES == (double*)(base + PINNED_BYTES), "the staged inputs end the block\n");
        CHECK((SMALL_MAX_N + 1) * SMALL_ADD_MAX_P == 771 && 771 <= SMALL_IN_DOUBLES, "add_sample's largest obs_mean\n");
        free(base);
    }
    if (fails)
        return 1;
    printf("shell layout ok: %zu + %zu bytes\n", DEV_BYTES, PINNED_BYTES);
    return 0;
}
