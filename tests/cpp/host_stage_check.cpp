// Stand-alone check of csrc/host_stage.h (no HIP, no library): the layouts the IK and the unicycle host forms state, against the offset
// chains those entry points wrote out by hand before the helper existed, and the helper's refusals.  Built with
// -fsanitize=address,undefined by tests/test_abi_host.py; the copies below run into blocks of exactly the layout's size, so a row
// that is too long for its place is an ASan report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "host_stage.h"

using wcqp::StageLayout;
using wcqp::StageSlot;

static int g_fail = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static int copy(void* dst, const void* src, size_t bytes) { std::memcpy(dst, src, bytes); return 0; }

// no two arrays overlap, every offset is a multiple of the element size, everything ends inside the block
static void check_rows(const StageLayout& st, const std::vector<size_t>& elem) {
    CHECK((size_t)st.n == elem.size());
    for (int a = 0; a < st.n; ++a) {
        CHECK(st.rows[a].off % elem[a] == 0);
        CHECK(st.rows[a].off + st.rows[a].bytes <= st.total);
        for (int b = a + 1; b < st.n; ++b)
            CHECK(st.rows[a].off + st.rows[a].bytes <= st.rows[b].off || st.rows[b].off + st.rows[b].bytes <= st.rows[a].off);
    }
}

// copy every input in, "run", copy every output out - through a heap block of exactly st.total bytes (ASan guards both ends)
static void round_trip(StageLayout& st) {
    std::vector<char> block(st.total);
    CHECK(st.copy_in(block.data(), block.size(), copy) == 0);
    for (int k = 0; k < st.n; ++k) {
        if (st.rows[k].src) CHECK(std::memcmp(block.data() + st.rows[k].off, st.rows[k].src, st.rows[k].bytes) == 0);
        else std::memset(block.data() + st.rows[k].off, 0x40 + k, st.rows[k].bytes);        // what a kernel would leave
    }
    CHECK(st.copy_out(copy) == 0);
    for (int k = 0; k < st.n; ++k)
        if (st.rows[k].dst && !st.rows[k].src)
            for (size_t i = 0; i < st.rows[k].bytes; ++i) CHECK(static_cast<const char*>(st.rows[k].dst)[i] == 0x40 + k);
}

// ---- wcqp_ik_solve_host: twelve arrays --------------------------------------------------------------------------------------------------
static void check_ik(size_t B, bool with_foot_err) {
    const size_t kNV = 29, kDof = 23, kStateLen = 87;
    std::vector<double> JL(B * 6 * kNV, 1.0), JR(B * 6 * kNV, 2.0), JN(B * 3 * kNV, 3.0), JC(B * 3 * kNV, 4.0), q(B * kDof, 5.0), state(B * kStateLen, 6.0);
    std::vector<double> dq(B * kDof), fe(B * 12);
    std::vector<int32_t> status(B), iters(B);
    std::vector<uint32_t> lo(B), up(B);
    double* foot_err = with_foot_err ? fe.data() : nullptr;
    StageLayout st;
    const auto d_jl = st.in(JL.data(), B * 6 * kNV), d_jr = st.in(JR.data(), B * 6 * kNV), d_jn = st.in(JN.data(), B * 3 * kNV), d_jc = st.in(JC.data(), B * 3 * kNV);
    const auto d_q = st.in(q.data(), B * kDof), d_s = st.in(state.data(), B * kStateLen);
    const auto d_dq = st.out(dq.data(), B * kDof), d_fe = st.out(foot_err, B * 12, true);
    const auto d_st = st.out(status.data(), B);
    const auto d_lo = st.out((uint32_t*)nullptr, B), d_up = st.out(up.data(), B);      // (active_lower not wanted back: it keeps its device array)
    const auto d_it = st.out(iters.data(), B);
    CHECK(!st.refused);
    // the chain the entry point wrote by hand (doubles, then four 32-bit rows)
    const size_t o_jl = 0, o_jr = o_jl + B * 6 * kNV, o_jn = o_jr + B * 6 * kNV, o_jc = o_jn + B * 3 * kNV,
                 o_q = o_jc + B * 3 * kNV, o_st = o_q + B * kDof, o_dq = o_st + B * kStateLen,
                 o_fe = o_dq + B * kDof, n_dbl = o_fe + B * 12;
    CHECK(st.offset(d_jl) == o_jl * 8 && st.offset(d_jr) == o_jr * 8 && st.offset(d_jn) == o_jn * 8 && st.offset(d_jc) == o_jc * 8);
    CHECK(st.offset(d_q) == o_q * 8 && st.offset(d_s) == o_st * 8 && st.offset(d_dq) == o_dq * 8);
    if (with_foot_err) {
        CHECK(st.n == 12 && st.offset(d_fe) == o_fe * 8);
        CHECK(st.offset(d_st) == n_dbl * 8 && st.offset(d_lo) == n_dbl * 8 + B * 4 && st.offset(d_up) == n_dbl * 8 + B * 8 && st.offset(d_it) == n_dbl * 8 + B * 12);
        CHECK(st.total == n_dbl * 8 + B * 4 * 4);
        check_rows(st, {8, 8, 8, 8, 8, 8, 8, 8, 4, 4, 4, 4});
    } else {
        // absent: no room, and the 32-bit rows move up behind dq
        CHECK(st.n == 11 && d_fe.row == -1);
        CHECK(st.offset(d_st) == o_fe * 8 && st.offset(d_it) == o_fe * 8 + B * 12);
        CHECK(st.total == o_fe * 8 + B * 4 * 4);
        check_rows(st, {8, 8, 8, 8, 8, 8, 8, 4, 4, 4, 4});
    }
    round_trip(st);
    CHECK((st[d_fe] == nullptr) == !with_foot_err);
    CHECK(st[d_lo] != nullptr && st[d_jl] == reinterpret_cast<double*>(st.base));
}

// ---- wcqp_unicycle_plan_host: ten arrays (eight when the planner keeps no step rows, K = 0) ------------------------------------------------
static void check_unicycle(size_t B, size_t K) {
    std::vector<double> left0(B * 12, 1.0), right0(B * 12, 2.0), goal(B * 2, 3.0), target(B * K * 3 + 1), dp(B * 2), ue(B * 3);
    std::vector<int32_t> n_steps(B), status(B);
    std::vector<uint8_t> first_side(B, 1), side(B * K + 1);
    StageLayout st;
    const auto d_l = st.in(left0.data(), B * 12), d_r = st.in(right0.data(), B * 12), d_g = st.in(goal.data(), B * 2);
    const auto d_t = st.out(target.data(), B * K * 3, true), d_dp = st.out(dp.data(), B * 2), d_ue = st.out((double*)nullptr, B * 3);
    const auto d_n = st.out(n_steps.data(), B), d_st = st.out(status.data(), B);
    const auto d_fs = st.in(first_side.data(), B);
    const auto d_sd = st.out(side.data(), B * K, true);
    CHECK(!st.refused);
    // the chain the entry point wrote by hand: doubles, then the 32-bit rows, then the bytes
    const size_t o_l = 0, o_r = o_l + B * 12, o_g = o_r + B * 12, o_t = o_g + B * 2, o_dp = o_t + B * K * 3, o_ue = o_dp + B * 2, n_d = o_ue + B * 3;
    const size_t bytes = n_d * 8 + 2 * B * 4 + B + B * K;
    CHECK(st.offset(d_l) == o_l * 8 && st.offset(d_r) == o_r * 8 && st.offset(d_g) == o_g * 8 && st.offset(d_dp) == o_dp * 8 && st.offset(d_ue) == o_ue * 8);
    CHECK(st.offset(d_n) == n_d * 8 && st.offset(d_st) == n_d * 8 + B * 4 && st.offset(d_fs) == n_d * 8 + 2 * B * 4);
    CHECK(st.total == bytes);
    if (K) {
        CHECK(st.n == 10 && st.offset(d_t) == o_t * 8 && st.offset(d_sd) == n_d * 8 + 2 * B * 4 + B);
        check_rows(st, {8, 8, 8, 8, 8, 8, 4, 4, 1, 1});
    } else {
        CHECK(st.n == 8 && d_t.row == -1 && d_sd.row == -1);
        check_rows(st, {8, 8, 8, 8, 8, 4, 4, 1});
    }
    round_trip(st);
    CHECK((st[d_t] == nullptr) == (K == 0) && (st[d_sd] == nullptr) == (K == 0));
    CHECK(st[d_ue] != nullptr);
}

// ---- refusals: a seventeenth array; an input without its host array; a fixed block one byte too small ------------------------------------
static void check_refusals() {
    const double src[4] = {1.0, 2.0, 3.0, 4.0};
    std::vector<char> block(16 * 32 + 64, 0x5a);
    {
        StageLayout st;
        for (int k = 0; k < 16; ++k) CHECK(st.in(src, 4).row == k);
        CHECK(!st.refused && st.total == 16 * 32 && st.fits(16 * 32));
        const auto extra = st.in(src, 4);
        CHECK(extra.row == -1 && st.refused && st.n == 16 && st.total == 16 * 32 && st[extra] == nullptr);
        CHECK(!st.fits(block.size()));
        CHECK(st.copy_in(block.data(), block.size(), copy) == wcqp::kStageRefused && st.base == nullptr);
        for (char c : block) CHECK(c == 0x5a);
    }
    {
        StageLayout st;
        st.in(src, 4);
        CHECK(st.in((const double*)nullptr, 4).row == -1 && st.refused);
        CHECK(st.copy_in(block.data(), block.size(), copy) == wcqp::kStageRefused);
        for (char c : block) CHECK(c == 0x5a);
    }
    {
        // the fixed kind: capacity from the same description with every array present; one byte less is refused and nothing is written
        StageLayout sizing;
        sizing.in(wcqp::stage_sizing<double>(), 4); sizing.in(wcqp::stage_sizing<double>(), 4, true); sizing.in(wcqp::stage_sizing<uint8_t>(), 3);
        CHECK(sizing.total == 67);
        StageLayout st;
        st.in(src, 4); st.in(src, 4, true); st.in(reinterpret_cast<const uint8_t*>(src), 3);
        CHECK(st.total == sizing.total);
        CHECK(st.copy_in(block.data(), sizing.total - 1, copy) == wcqp::kStageRefused && st.base == nullptr);
        for (char c : block) CHECK(c == 0x5a);
        std::vector<char> exact(sizing.total);
        CHECK(st.copy_in(exact.data(), exact.size(), copy) == 0);
        StageLayout fewer;      // an optional array left out: fits the same block with room to spare
        fewer.in(src, 4); fewer.in((const double*)nullptr, 4, true); fewer.in(reinterpret_cast<const uint8_t*>(src), 3);
        CHECK(!fewer.refused && fewer.total == 35 && fewer.copy_in(exact.data(), exact.size(), copy) == 0);
    }
}

int main() {
    for (size_t B : {1, 3, 5, 67}) {
        check_ik(B, true);
        check_ik(B, false);
        check_unicycle(B, 0);
        check_unicycle(B, 4);
    }
    check_refusals();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("host_stage ok\n");
    return 0;
}
