"""The LSD launch geometry (lsd_geometry in fd_rt_lsd.cpp, the kernels' strip and pass counts in fd_lsd.hip),
restated for the tests: a test asserts from these formulas the branch its shape is meant to take, so that a later
geometry change cannot silently move it off the boundary."""


def lsd_chunks(batch, rows, cols):
    """(chunk_h, chunks): 16-row chunks while 32-row chunks would leave fewer than 4096 map waves."""
    strips4 = (cols - 1 + 255) // 256
    chunk_h = 16 if batch * strips4 * ((rows - 3 + 31) // 32) < 4096 else 32
    return chunk_h, (rows - 3 + chunk_h - 1) // chunk_h


def lsd_columns(cols):
    """(k_lsd_map's 256-column strips, how many of them take the INTERIOR tile, k_lsd_scan's passes of 1024
    columns, k_lsd_scatter's 32-column wave strips)."""
    strips4 = (cols - 1 + 255) // 256
    interior = sum(1 for s in range(strips4) if s * 256 >= 1 and s * 256 + 255 <= cols - 3)
    return strips4, interior, (cols - 1 + 1023) // 1024, (cols - 1 + 31) // 32
