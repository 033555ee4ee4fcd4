// mppi_launch_tile.hip — instantiates k_rollout_tile for ONE action dimension (-DMPPI_UNIT_A): 3 tile sizes x 2 Q forms x
// 7 (noise source, mode) pairs = 42 kernels per object.
#include "mppi_handle.hip.h"
#ifndef MPPI_UNIT_A
#error "compile with -DMPPI_UNIT_A=<action dimension 1..4> (mppi-tf_amd/build.py)"
#endif

struct TilePick {
    decltype(&k_rollout_tile<MPPI_UNIT_A, 64, false, SRC_PHILOX, MODE_ROLLOUT>) kern; // nullptr: no instance serves (src, mode)
    const char *name;
};

template <int A, int R, bool QFULL, int SRC, int MODE>
static TilePick tile_inst()
{
    static const std::string name = mppi_fmt("mppi::k_rollout_tile<%d, %d, %s, %d, %d>", A, R, mppi_tf(QFULL), SRC, MODE);
    return {k_rollout_tile<A, R, QFULL, SRC, MODE>, name.c_str()};
}

template <int A, int R, bool QFULL>
static TilePick tile_mode(int src, int mode)
{
#define MPPI_TILE_CASE(SRC, MODE) \
    if (src == SRC && mode == MODE) return tile_inst<A, R, QFULL, SRC, MODE>();
    MPPI_TILE_CASE(SRC_PHILOX, MODE_ROLLOUT)
    MPPI_TILE_CASE(SRC_HBM, MODE_ROLLOUT)
    MPPI_TILE_CASE(SRC_PHILOX, MODE_COSTS_GIVEN)
    MPPI_TILE_CASE(SRC_HBM, MODE_COSTS_GIVEN)
    MPPI_TILE_CASE(SRC_PHILOX, MODE_COST_ONLY)
    MPPI_TILE_CASE(SRC_HBM, MODE_COST_ONLY)
    MPPI_TILE_CASE(SRC_PHILOX, MODE_NOISE_ONLY)
#undef MPPI_TILE_CASE
    return {nullptr, nullptr};
}

static TilePick pick_tile(const mppi_handle *h, int src, int mode)
{
    constexpr int A = MPPI_UNIT_A;
    const bool qf = h->hc.q_full != 0;
    if (h->R == 64) return qf ? tile_mode<A, 64, true>(src, mode) : tile_mode<A, 64, false>(src, mode);
    if (h->R == 32) return qf ? tile_mode<A, 32, true>(src, mode) : tile_mode<A, 32, false>(src, mode);
    if (h->R == 16) return qf ? tile_mode<A, 16, true>(src, mode) : tile_mode<A, 16, false>(src, mode);
    return {nullptr, nullptr};
}

// (no kernel events: a profiled step records its events around this launch)
hipError_t MPPI_CAT(mppi_tile_a, MPPI_UNIT_A)(MPPI_TILE_PARAMS)
{
    const TilePick p = pick_tile(h, src, mode);
    if (!p.kern) return hipErrorInvalidValue;
    if (hipError_t e = mppi_raise_lds_ceiling(reinterpret_cast<const void *>(p.kern), h->device, h->tile_lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(p.kern, dim3(h->nb), dim3(kThreads), h->tile_lds, st, consts, x_dev, U_dev, eps, h->d_step, cost, part, noise_out, 1, h->nbp);
    return hipGetLastError();
}

const char *MPPI_CAT(mppi_tile_name_a, MPPI_UNIT_A)(const mppi_handle *h, int src, int mode) { return pick_tile(h, src, mode).name; }
