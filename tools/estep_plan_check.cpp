// estep_plan_check.cpp -- the E-step plan builders of csrc/tmvb_estep_plan.h on the host alone, for a sanitizer build (no device is touched):
//   hipcc -std=c++17 --cuda-host-only -Xarch_host -fsanitize=address,undefined -I include -I topicmodelsvb.jl_amd/csrc tools/estep_plan_check.cpp -o /tmp/estep_plan_check
// Builds the LDA and the CTPF plan of three corpora -- the length classes of tests/test_ctpf_gpu.py::test_long_documents_and_the_lane_per_token_path, no document,
// one document -- for every path flag, prints them and checks that the records tile the processing order and that the order is a permutation;
// then the subsets of that test's classes: each must hold the launch kind it is there for (one four-wave class alone, one tile count alone, no launch on aux[0]).
#include "tmvb_estep_plan.h"

void tmvb_set_error(const char*, ...) {}

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; std::printf("FAILED %s (line %d)\n", #cond, __LINE__); } } while (0)

template <class L>
static void check_tiling(const std::vector<int32_t>& order, const std::vector<L>& plan, size_t M)
{
    std::vector<int> seen(M, 0);
    CHECK(order.size() == M);
    for (int32_t d : order) { CHECK(d >= 0 && (size_t)d < M); if (d >= 0 && (size_t)d < M) ++seen[(size_t)d]; }
    for (int s : seen) CHECK(s == 1);
    int64_t pos = 0;
    for (const L& b : plan) { CHECK(b.first == pos && b.count > 0); pos = b.first + b.count; }
    CHECK(pos == (int64_t)M);
}

static void lda_case(const char* name, const std::vector<int64_t>& len, int K, bool grid, bool one_launch, bool two_copy, int P)
{
    const int KP = tmvb_kpad(K);
    lda_plan_flags f;
    f.reg_path = K <= 128 && lda_reg_lpr_supported(KP / 4); f.grid_path = f.reg_path && grid; f.one_launch = f.reg_path && KP <= 60 && P == 1 && one_launch;
    f.two_copy = two_copy && KP <= 60;
    std::vector<int32_t> order, doc_piece;
    std::vector<lda_launch> plan;
    lda_build_plan(len, KP, f, order, plan);
    if (P > 1) lda_cut_pieces(len, std::accumulate(len.begin(), len.end(), (int64_t)0), order, P, plan, doc_piece);
    std::printf("lda %s K=%d grid=%d one=%d tt=%d P=%d:", name, K, (int)f.grid_path, (int)f.one_launch, (int)f.two_copy, P);
    int piece = 0;
    for (const lda_launch& b : plan) {
        std::printf(" [kind %d role %d %lld+%lld n%d w%d rows%d p%d]", (int)b.kind, (int)b.role, (long long)b.first, (long long)b.count, b.n, b.waves, b.tile_rows, b.piece);
        if (b.role == tmvb_role::CHAIN) { CHECK(b.piece >= piece && b.piece < P); piece = b.piece; } else CHECK(b.piece == (P > 1 ? P - 1 : 0));
        for (int64_t q = b.first; P > 1 && q < b.first + b.count; ++q) CHECK(doc_piece[(size_t)order[(size_t)q]] == b.piece);
    }
    std::printf("\n");
    check_tiling(order, plan, len.size());
}

static std::vector<ctpf_launch> ctpf_case(const char* name, const std::vector<int64_t>& n, const std::vector<int64_t>& r, int K, bool grid)
{
    const int KP = tmvb_kpad(K);
    const bool reg_path = KP / 4 <= 15 && ((KP / 4) & 1);
    std::vector<int32_t> order;
    std::vector<ctpf_launch> plan;
    ctpf_build_plan(n, r, KP, reg_path, reg_path && grid, order, plan);
    std::printf("ctpf %s K=%d grid=%d:", name, K, (int)(reg_path && grid));
    for (const ctpf_launch& b : plan) {
        std::printf(" [kind %d role %d %lld+%lld a%d n%d (%d,%d) w%d rows%d]", (int)b.kind, (int)b.role, (long long)b.first, (long long)b.count, b.count_a, b.n, b.npt, b.npr,
                    b.waves, b.tile_rows);
        if (b.kind == ctpf_kind::GRID_LONG2) CHECK(b.count_a > 0 && b.count_a < b.count);
        for (int64_t q = b.first; q < b.first + b.count; ++q) {       // every document sits in a launch whose kernel holds it
            const int64_t nd = n[(size_t)order[(size_t)q]], rd = r[(size_t)order[(size_t)q]];
            const ctpf_grid_cls c = ctpf_grid_class(nd, rd);
            if (b.kind == ctpf_kind::GRID_NARROW) CHECK(c.waves == 1 && c.npt < 4);
            if (b.kind == ctpf_kind::GRID_WIDE) CHECK(c.waves == 1 && c.npt >= 4);
            if (b.kind == ctpf_kind::GRID_LONG) CHECK(c.waves == 4 && c.npt == b.npt && c.npr == b.npr);
            if (b.kind == ctpf_kind::GRID_LONG2) CHECK(c.waves == 4 && c.npt == (q - b.first < b.count_a ? 3 : 2));
            if (b.kind == ctpf_kind::REG) CHECK(nd <= 64 * b.n && rd <= 64 && (b.n == 1 || nd > 64));
            if (b.kind == ctpf_kind::REG_ANY) CHECK(nd <= 128 && rd <= 64);
        }
    }
    std::printf("\n");
    check_tiling(order, plan, n.size());
    return plan;
}

// the subsets of tests/test_ctpf_gpu.py (LONG_SUBSETS) reach the launch kinds that the whole class corpus merges away
static void ctpf_subsets(const std::vector<std::pair<int64_t, int64_t>>& shapes)
{
    auto plan_of = [&](const char* name, bool grid, auto keep) {
        std::vector<int64_t> n, r;
        for (const auto& s : shapes) if (keep(s.first, s.second) || (s.first == 600 && s.second == 50) || (s.first == 5 && s.second == 600)) { n.push_back(s.first); r.push_back(s.second); }
        return ctpf_case(name, n, r, 50, grid);
    };
    auto count = [](const std::vector<ctpf_launch>& plan, ctpf_kind kind) { int c = 0; for (const ctpf_launch& b : plan) c += b.kind == kind; return c; };
    auto beside = [](const std::vector<ctpf_launch>& plan) { int c = 0; for (const ctpf_launch& b : plan) c += b.role == tmvb_role::BESIDE; return c; };
    auto cls = [](int64_t n, int64_t r) { return ctpf_grid_class(n, r); };
    std::vector<ctpf_launch> p = plan_of("all", true, [](int64_t, int64_t) { return true; });
    CHECK(count(p, ctpf_kind::GRID_LONG2) == 1 && count(p, ctpf_kind::GRID_LONG) == 0 && count(p, ctpf_kind::GRID_NARROW) == 1 && count(p, ctpf_kind::GRID_WIDE) == 1 && beside(p) == 1);
    for (const ctpf_launch& b : p) if (b.kind == ctpf_kind::GRID_LONG2) CHECK(b.count_a == 2 && b.count == 6 && b.npt == 0 && b.npr == 0 && b.role == tmvb_role::LONG);
    p = plan_of("no33", true, [&](int64_t n, int64_t r) { return !(cls(n, r).waves == 4 && cls(n, r).npt == 3); });
    CHECK(count(p, ctpf_kind::GRID_LONG2) == 0 && count(p, ctpf_kind::GRID_LONG) == 1);
    for (const ctpf_launch& b : p) if (b.kind == ctpf_kind::GRID_LONG) CHECK(b.npt == 2 && b.npr == 4 && b.count == 4 && b.waves == 4);
    p = plan_of("no24", true, [&](int64_t n, int64_t r) { return !(cls(n, r).waves == 4 && cls(n, r).npt == 2); });
    CHECK(count(p, ctpf_kind::GRID_LONG2) == 0 && count(p, ctpf_kind::GRID_LONG) == 1);
    for (const ctpf_launch& b : p) if (b.kind == ctpf_kind::GRID_LONG) CHECK(b.npt == 3 && b.npr == 3 && b.count == 2 && b.waves == 4);
    p = plan_of("narrow", true, [&](int64_t n, int64_t r) { return cls(n, r).waves == 1 && cls(n, r).npt < 4; });
    CHECK(count(p, ctpf_kind::GRID_NARROW) == 1 && count(p, ctpf_kind::GRID_WIDE) == 0 && count(p, ctpf_kind::GRID_LONG) + count(p, ctpf_kind::GRID_LONG2) == 0 && beside(p) == 0);
    p = plan_of("wide", true, [&](int64_t n, int64_t r) { return cls(n, r).waves == 1 && cls(n, r).npt >= 4; });
    CHECK(count(p, ctpf_kind::GRID_WIDE) == 1 && count(p, ctpf_kind::GRID_NARROW) == 0 && beside(p) == 1);
    p = plan_of("wide", false, [&](int64_t n, int64_t r) { return cls(n, r).waves == 1 && cls(n, r).npt >= 4; });
    CHECK(count(p, ctpf_kind::REG) == 1 && count(p, ctpf_kind::REG_ANY) == 0);
    for (const ctpf_launch& b : p) if (b.kind == ctpf_kind::REG) CHECK(b.n == 2 && b.count == 3);
    p = plan_of("short", false, [](int64_t n, int64_t r) { return n <= 64 && r <= 3; });
    CHECK(count(p, ctpf_kind::REG) == 1 && count(p, ctpf_kind::REG_ANY) == 0);
    for (const ctpf_launch& b : p) if (b.kind == ctpf_kind::REG) CHECK(b.n == 1 && b.count == 3);
    p = plan_of("all", false, [](int64_t, int64_t) { return true; });
    CHECK(count(p, ctpf_kind::REG_ANY) == 1 && count(p, ctpf_kind::REG) == 0);
}

int main()
{
    const std::vector<std::pair<int64_t, int64_t>> shapes = {{30, 3}, {64, 1}, {90, 20}, {128, 32}, {129, 5}, {192, 30}, {100, 40}, {128, 64}, {60, 100}, {250, 10},
                                                             {200, 300}, {20, 500}, {300, 200}, {380, 380}, {600, 50}, {10, 0}, {5, 600}};
    std::vector<int64_t> n, r;
    for (const auto& s : shapes) { n.push_back(s.first); r.push_back(s.second); }
    std::vector<int64_t> lda_len = n;                                  // LDA: the term counts, and the long classes of its own kernels
    for (int64_t extra : {700, 769, 1100, 3000, 9000}) lda_len.push_back(extra);
    const struct { const char* name; std::vector<int64_t> n, r; } corpora[] = {{"classes", n, r}, {"empty", {}, {}}, {"one", {100}, {7}}};
    for (const auto& c : corpora) {
        for (int K : {7, 50, 100, 130})
            for (int grid = 0; grid < 2; ++grid)
                for (int P : {1, 2, 3}) {
                    const std::vector<int64_t>& len = std::string(c.name) == "classes" ? lda_len : c.n;
                    lda_case(c.name, len, K, grid, true, false, P);
                    if (P == 1) { lda_case(c.name, len, K, grid, false, false, P); lda_case(c.name, len, K, grid, false, true, P); }
                }
        for (int K : {7, 50, 100})
            for (int grid = 0; grid < 2; ++grid) ctpf_case(c.name, c.n, c.r, K, grid);
    }
    ctpf_subsets(shapes);
    std::printf("%s (%d failed checks)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
