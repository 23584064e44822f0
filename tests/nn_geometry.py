"""The SuperPoint layer kernels' launch geometry (launch_conv3x3_c64, launch_conv3x3_c1_bias_relu and
launch_bias_relu in fd_nn_act.hip; launch_nn_heat_softmax and launch_nn_desc_normalize in fd_nn.hip, with the
index arithmetic of their kernels), restated for the tests: a test asserts from these formulas the branch its
shape is meant to take, so that a later geometry change cannot silently move it off that branch."""
from collections import Counter

K10_ROWS, K10_COLS, K10_GRID = 8, 32, 256  # kPpRows, kPpCols, the persistent grid (one workgroup per CU)
K9_MAX_W, K9_GRID = 4096, 256 * 32  # kConv1MaxW, launch_conv3x3_c1_bias_relu's row grid
K9_CHANNELS = (8, 16, 32, 64, 128, 256)
ACT_GRID = 256 * 64  # launch_bias_relu's block limit (256 threads, one 8-channel vector each per trip)
HEAT_CELLS = 32  # kHeatCells


def k10_tiles(n, h, w):
    """(tiles per frame down, across, in all): 8 x 32-pixel tiles, ragged at the frame's bottom and right."""
    th, tw = -(-h // K10_ROWS), -(-w // K10_COLS)
    return th, tw, n * th * tw


def k10_first_tile(b, grid):
    """L(b): the first tile of workgroup b; the full grid deals neighbouring tiles to one XCD's workgroups."""
    return (b & 7) * 32 + (b >> 3) if grid == K10_GRID else b


def k10_depths(n, h, w):
    """K of every workgroup, by block index: workgroup b runs tiles k G + L(b), k < K."""
    total = k10_tiles(n, h, w)[2]
    grid = min(total, K10_GRID)
    out = []
    for b in range(grid):
        first = k10_first_tile(b, grid)
        out.append(-(-(total - first) // grid) if first < total else 0)
    return out


def k10_depth_counts(n, h, w):
    """The multiset of K over the grid, as {K: workgroups}."""
    return dict(Counter(k10_depths(n, h, w)))


def k9_geometry(n, h, w, c):
    """dict(grid, trips, per, steps): the row grid, the most rows one workgroup takes, the pixels a block step
    covers (256 threads / (c / 8) channel groups) and the steps of one row."""
    assert c in K9_CHANNELS and w <= K9_MAX_W
    rows = n * h
    grid = min(rows, K9_GRID)
    per = 256 // (c // 8)
    return dict(grid=grid, trips=-(-rows // grid) if grid else 0, per=per, steps=-(-w // per))


def bias_relu_geometry(n, h, w, c, pool):
    """dict(vectors, grid, trips): output 8-channel vectors, blocks and the most grid-stride trips of a thread."""
    vec = n * h * w * (c // 8)
    out = vec // 4 if pool else vec
    grid = min(-(-out // 256), ACT_GRID)
    return dict(vectors=out, grid=grid, trips=-(-out // (grid * 256)) if grid else 0)


def heat_groups(wc):
    """(workgroups per cell row, cells of the last one): k_nn_heat_softmax takes 32 cells of one row."""
    g = -(-wc // HEAT_CELLS)
    return g, wc - (g - 1) * HEAT_CELLS


def desc_geometry(cells, c):
    """dict(span, per_wave, rounds, waves, idle): lanes per cell, cells per wave, 8-channel rounds of a lane,
    waves launched (4 per block) and the cell slots of the last wave that hold no cell."""
    groups = c // 8
    span = 8 if groups <= 8 else 16 if groups <= 16 else 32 if groups <= 32 else 64
    per_wave = 64 // span
    waves = -(-cells // per_wave)
    return dict(span=span, per_wave=per_wave, rounds=-(-groups // span), waves=waves, idle=waves * per_wave - cells)
