"""Plain-Python restatement of the forward pass's scheduling rules as they stood at commit 6dcf15b, before the host layer got its one
route (csrc/fc_forward_route.hpp) and its one schedule function (csrc/fc_tile.hpp: tile_schedule).  Transcribed line by line from that
commit, to be diffed by eye against it:

  edge_parts_log2     fc_tile.hpp: edge_parts_log2
  ring_major          fc_forward_ring.hip: ring_enabled, forward_ring_fits (the threshold; plan_ring taken to fit, see below)
  schedule, dense / frequency-major
                      fc_forward_kernels.hpp: forward_impl_mode (nvt, grid) and fc_tile.hpp: tile_items
  schedule, ring-major
                      fc_forward_ring.hip: forward_ring_impl (grid, rem, the last round's halves, spread_cus)
  image sizes         fc_tile.hpp: make_mma_geom, packed_image_floats; fc_forward_ring.hip: packed_ring_image_floats

All development switches at their defaults (FC_RING, FC_RING_HALVES, FC_HALF_TILES, FC_EDGE_PARTS_MAX unset).  Modes as in fc_dims::mode:
0 split-f16 (two halves per operand), 1 f32 (none), 2 f16 (one).
"""

TILE = 16
HALVES_OF_MODE = {0: 2, 1: 0, 2: 1}


def edge_parts_log2(N, E, cus, cap=3):
    if N <= 0:
        return 0
    ntiles = (N + TILE - 1) // TILE
    deg = E // N
    pl = 0
    while pl < cap and (ntiles << (pl + 1)) <= cus and (deg >> (pl + 1)) >= 8:
        pl += 1
    return pl


def ring_major(N, kind, mode, cus):
    """forward_impl's `kind != 0 && forward_ring_fits(d)` for a shape whose ring-major LDS plan fits (plan_ring(...).ok: true of every
    shape up to 64 channels at band limits 1..3 in the default mode; the callers of this file use (16, 16, 4, 1) and (64, 64, 6, 3))."""
    return kind != 0 and HALVES_OF_MODE[mode] == 2 and (N + TILE - 1) // TILE > cus


def tile_items(ntiles, grid, parts_log2):
    nv_full = nv_total = ntiles << parts_log2
    if parts_log2 != 0 or grid <= 0:
        return nv_full, nv_total
    rem = ntiles % grid
    if ntiles > grid and rem > 0 and 2 * rem <= grid:
        nv_full = ntiles - rem
        nv_total = nv_full + 2 * rem
    return nv_full, nv_total


def schedule(N, E, kind, mode, cus):
    """-> dict(arrangement, parts, grid, whole, half, spread) of the launch forward_impl makes when it is given its workspace."""
    ntiles = (N + TILE - 1) // TILE
    parts_log2 = 0 if kind == 0 else edge_parts_log2(N, E, cus)
    nvt = ntiles << parts_log2
    spread = 0
    if ring_major(N, kind, mode, cus):
        grid = nvt if nvt < 2 * cus else 2 * cus
        rem = nvt % grid
        nv_full = nv_total = nvt
        if parts_log2 == 0 and rem > 0 and 2 * rem <= grid:
            nv_full = nvt - rem
            nv_total = nv_full + 2 * rem
        if parts_log2 == 0 and cus < nvt < 2 * cus:
            nv_full = 2 * nvt - 2 * cus
            nv_total = 2 * cus
            spread = 1
            grid = 2 * cus
        arrangement = 'ring-major'
    else:
        factored = kind != 0
        grid = (nvt if nvt < cus else cus) if factored else ntiles
        nv_full, nv_total = tile_items(ntiles, grid if factored else 0, parts_log2)
        arrangement = 'frequency-major'
    return dict(arrangement=arrangement, parts=1 << parts_log2, grid=grid, whole=nv_full, half=nv_total - nv_full, spread=spread)


def _round_up(a, b):
    return (a + b - 1) // b * b


def _mp_kp(M, R, channels, halves):
    """make_mma_geom's MP and KP; the ring-major geometry (ring_geom) is the same with F in the place of R."""
    ki = _round_up(channels, 8) if halves else channels
    return _round_up(M, 16), _round_up(R * ki, 32 if halves else 16)


def frequency_image_floats(I, O, R, B, mode):
    halves, F = HALVES_OF_MODE[mode], 2 * B + 1
    mp, kp = _mp_kp(O, R, I, halves)
    return mp + F * halves * mp * kp if halves else F * 2 * mp * kp


def ring_image_floats(I, O, R, B, mode):
    halves, F = HALVES_OF_MODE[mode], 2 * B + 1
    mp, kp = _mp_kp(O, F, I, halves)
    return mp + R * halves * mp * kp
