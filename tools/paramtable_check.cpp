// Checks ParamTable of surfd_amd/csrc/paramtable.h on the host: add / info / match / mark / first_missing, every refusal of
// match with its message.  Stand-alone (its own set_error), host code only (hipcc --cuda-host-only, for the HIP headers common.h
// needs); tests/test_paramtable_cpu.py builds it with the host sanitizers and runs it.  Exit status 0: every check held.
#include "../surfd_amd/csrc/common.h"
#include "../surfd_amd/csrc/paramtable.h"
#include <cstring>

static char g_err[512];

namespace surfd {
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace surfd

using namespace surfd;

static int g_failed = 0;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("line %d: %s   [last error: %s]\n", __LINE__, #cond, g_err); \
            ++g_failed;                                                      \
        }                                                                    \
    } while (0)

static bool says(const char *a, const char *b = "", const char *c = "") { return strstr(g_err, a) && strstr(g_err, b) && strstr(g_err, c); }

int main() {
    ParamTable t;
    // ranks 0 to 4, one ignored entry in the middle, then a few hundred keys
    CHECK(t.add("r0", {}) == 0);
    CHECK(t.add("r1", {7}, 11) == 1);
    CHECK(t.add("bn.num_batches_tracked", {}, 0, true) == 2);
    CHECK(t.add("r2", {3, 5}, 22) == 3);
    CHECK(t.add("r3", {2, 3, 4}) == 4);
    CHECK(t.add("r4", {2, 1, 3, 6}, -4) == 5);
    const int many = 300;
    for (int i = 0; i < many; ++i) CHECK(t.add("blocks." + std::to_string(i) + ".weight", {i + 1, 2}, 1000 + i) == 6 + i);
    CHECK(t.size() == 6 + many);
    CHECK(t.numel(0) == 1 && t.numel(1) == 7 && t.numel(2) == 1 && t.numel(3) == 15 && t.numel(4) == 24 && t.numel(5) == 36);
    CHECK(t[1].tag == 11 && t[5].tag == -4 && t[6 + 299].tag == 1299 && t[2].ignored && !t[3].ignored);

    // info: both ends, and every null
    const char *key = nullptr;
    int64_t shape[4] = {-1, -1, -1, -1};
    int ndim = -1;
    CHECK(param_info(&t, "who", 0, &key, shape, &ndim) == SURFD_OK && !strcmp(key, "r0") && ndim == 0 && shape[0] == -1);
    CHECK(param_info(&t, "who", t.size() - 1, &key, shape, &ndim) == SURFD_OK && !strcmp(key, "blocks.299.weight") && ndim == 2 &&
          shape[0] == 300 && shape[1] == 2 && shape[2] == -1);
    CHECK(param_info(&t, "who", 5, &key, shape, &ndim) == SURFD_OK && ndim == 4 && shape[0] == 2 && shape[1] == 1 && shape[2] == 3 && shape[3] == 6);
    CHECK(param_info(&t, "who", -1, &key, shape, &ndim) == SURFD_ERR_ARG && says("who"));
    CHECK(param_info(&t, "who", t.size(), &key, shape, &ndim) == SURFD_ERR_ARG);
    CHECK(param_info(nullptr, "who", 0, &key, shape, &ndim) == SURFD_ERR_ARG);
    CHECK(param_info(&t, "who", 0, nullptr, shape, &ndim) == SURFD_ERR_ARG);
    CHECK(param_info(&t, "who", 0, &key, nullptr, &ndim) == SURFD_ERR_ARG);
    CHECK(param_info(&t, "who", 0, &key, shape, nullptr) == SURFD_ERR_ARG);

    // match: every key with its own shape, in table order and out of it
    int w = -7;
    for (int i = t.size() - 1; i >= 0; --i) {
        CHECK(t.match("m", t[i].key.c_str(), t[i].shape, t[i].ndim, &w) == SURFD_OK && w == i);
    }
    CHECK(t.match("m", "r0", nullptr, 0, &w) == SURFD_OK && w == 0);                       // rank 0 needs no shape
    CHECK(t.match("m", "bn.num_batches_tracked", nullptr, 0, &w) == SURFD_OK && w == 2);   // ignored: matched like any other
    // match: the refusals; *which is left alone
    w = -7;
    const int64_t s35[2] = {3, 5}, s36[2] = {3, 6}, s45[2] = {4, 5}, s2136[4] = {2, 1, 3, 6}, s2137[4] = {2, 1, 3, 7};
    CHECK(t.match("m", nullptr, s35, 2, &w) == SURFD_ERR_ARG && says("m:", "null key"));
    CHECK(t.match("m", "r9", s35, 2, &w) == SURFD_ERR_ARG && says("m:", "unknown key", "'r9'"));
    CHECK(t.match("m", "", s35, 2, &w) == SURFD_ERR_ARG && says("unknown key"));
    CHECK(t.match("m", "R2", s35, 2, &w) == SURFD_ERR_ARG && says("unknown key", "'R2'"));
    CHECK(t.match("m", "r2", s35, 1, &w) == SURFD_ERR_ARG && says("'r2'", "rank 1", "expected 2"));
    CHECK(t.match("m", "r2", s35, 3, &w) == SURFD_ERR_ARG && says("'r2'", "rank 3", "expected 2"));
    CHECK(t.match("m", "r0", s35, 1, &w) == SURFD_ERR_ARG && says("'r0'", "rank 1", "expected 0"));
    CHECK(t.match("m", "bn.num_batches_tracked", s35, 1, &w) == SURFD_ERR_ARG && says("num_batches_tracked", "rank 1", "expected 0"));
    CHECK(t.match("m", "r2", s35, -1, &w) == SURFD_ERR_ARG && says("rank -1"));
    CHECK(t.match("m", "r4", s2136, 5, &w) == SURFD_ERR_ARG && says("'r4'", "rank 5", "expected 4"));
    CHECK(t.match("m", "r2", nullptr, 2, &w) == SURFD_ERR_ARG && says("'r2'", "null shape"));
    CHECK(t.match("m", "r2", s36, 2, &w) == SURFD_ERR_ARG && says("'r2'", "dim 1 is 6", "expected 5"));
    CHECK(t.match("m", "r2", s45, 2, &w) == SURFD_ERR_ARG && says("'r2'", "dim 0 is 4", "expected 3"));
    CHECK(t.match("m", "r4", s2137, 4, &w) == SURFD_ERR_ARG && says("'r4'", "dim 3 is 7", "expected 6"));
    CHECK(w == -7);
    CHECK(t.match("m", "r4", s2136, 4, &w) == SURFD_OK && w == 5);

    // first_missing: table order, ignored entries skipped, whether or not they were marked
    CHECK(!t.all_set() && t.first_missing() == 0);
    CHECK(t.require_all("fin") == SURFD_ERR_STATE && says("fin:", "'r0'", "was not set"));
    t.mark(0);
    CHECK(t.first_missing() == 1);
    t.mark(3);
    CHECK(t.first_missing() == 1);
    t.mark(1);
    CHECK(t.first_missing() == 4);                        // past the ignored entry 2 and the marked entry 3
    t.mark(2);
    CHECK(t.first_missing() == 4 && t[2].is_set);
    for (int i = t.size() - 1; i >= 5; --i) t.mark(i);
    CHECK(!t.all_set() && t.first_missing() == 4);
    CHECK(t.require_all("fin") == SURFD_ERR_STATE && says("'r3'", "not set"));
    t.mark(4);
    CHECK(t.all_set() && t.first_missing() == -1 && t.require_all("fin") == SURFD_OK);

    ParamTable only_ignored;
    only_ignored.add("a.num_batches_tracked", {}, 0, true);
    CHECK(only_ignored.all_set() && only_ignored.require_all("fin") == SURFD_OK);
    ParamTable empty;
    CHECK(empty.size() == 0 && empty.all_set());
    CHECK(param_info(&empty, "who", 0, &key, shape, &ndim) == SURFD_ERR_ARG);

    if (g_failed) printf("%d checks failed\n", g_failed);
    else printf("paramtable_check: OK\n");
    return g_failed ? 1 : 0;
}
