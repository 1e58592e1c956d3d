// sanitize_options_driver.cpp — grail_set_option / grail_get_option under AddressSanitizer + UBSan, and their transcript.
// Built by tests/test_sanitizers.py from grail-rs_amd/csrc/{options,voice_analysis,voice_host}.cpp and the planner's units with g++
// (those units make no HIP call); the error helpers of grail_api.cpp are defined here.  Neither entry point needs a
// device: a default-constructed grail_ctx that plans for 256 compute units suffices (as grail_plan_blocks has one).  The
// context owns its HIP resources by type, so its destructor names HIP entry points: tests/fake_hip.h defines them, and
// the driver checks that the context called none of them from construction to destruction.
// argv: the option names to walk (the test passes the names of the header's option block, in the header's order).  Every
// name, then a few the header does not list, is set to each probe value and read back; the return codes, the message of
// a failure, the value read and the context's options_epoch go to stdout, then every name is read once more.  What the
// option code did before it became a table is kept in tests/golden/options_transcript.txt: the output must equal it.
#include <cinttypes>

#include "../grail-rs_amd/csrc/api_internal.hpp"
#include "fake_hip.h"

// ---- the error helpers of grail_api.cpp
namespace grail {
namespace host {
static thread_local std::string g_err;
int fail(int status, const std::string &msg)
{
    g_err = msg;
    return status;
}
int hip_fail(hipError_t, const char *what) { return fail(GRAIL_ERR_HIP, what); }
std::string &last_error() { return g_err; }
}  // namespace host
}  // namespace grail
extern "C" const char *grail_last_error(void) { return grail::host::g_err.c_str(); }
// ----

static const int64_t PROBES[] = {-2, -1, 0, 1, 2, 3, 4, 5, 8, 64, 65, 1000, 1001, 4096, 4097, 2147483647ll, 2147483648ll};
static const char *const EXTRA[] = {"compute_units", "scan_debug", "no_such_option", "arithmetic ", ""};

static void read_back(grail_ctx *ctx, const char *name)
{
    int64_t v = -999;                      // (a refused read leaves it alone)
    const int rc = grail_get_option(ctx, name, &v);
    std::printf("get %d %" PRId64, rc, v);
    if (rc) std::printf(" \"%s\"", grail_last_error());
}

static void walk_options(int argc, char **argv)
{
    grail_ctx ctx;
    ctx.cus = ctx.device_cus = 256;
    std::vector<const char *> names(argv + 1, argv + argc);
    names.insert(names.end(), std::begin(EXTRA), std::end(EXTRA));
    int64_t v = 0;
    const auto refused = [](const char *what, const int rc) { std::printf("%s: %d \"%s\"\n", what, rc, grail_last_error()); };
    refused("set, ctx NULL", grail_set_option(nullptr, "arithmetic", 0));
    refused("get, ctx NULL", grail_get_option(nullptr, "arithmetic", &v));
    refused("set, name NULL", grail_set_option(&ctx, nullptr, 0));
    refused("get, name NULL", grail_get_option(&ctx, nullptr, &v));
    refused("get, value NULL", grail_get_option(&ctx, "arithmetic", nullptr));
    std::printf("epoch %" PRIu64 "\n", ctx.options_epoch);
    for (const char *name : names) {
        std::printf("[%s] ", name);
        read_back(&ctx, name);
        std::printf("\n");
        for (const int64_t probe : PROBES) {
            const int rc = grail_set_option(&ctx, name, probe);
            std::printf("  set %" PRId64 " %d", probe, rc);
            if (rc) std::printf(" \"%s\"", grail_last_error());
            std::printf(", ");
            read_back(&ctx, name);
            std::printf(", epoch %" PRIu64 "\n", ctx.options_epoch);
        }
    }
    std::printf("[at the end]\n");
    for (const char *name : names) {
        std::printf("  %s: ", name);
        read_back(&ctx, name);
        std::printf("\n");
    }
}

int main(int argc, char **argv)
{
    walk_options(argc, argv);
    if (!fake_hip::state().log.empty()) {
        std::fprintf(stderr, "a grail_ctx that was given no HIP resource made HIP calls: %s\n", fake_hip::names_since(0).c_str());
        return 1;
    }
    std::printf("sanitize options driver: ok\n");
    return 0;
}
