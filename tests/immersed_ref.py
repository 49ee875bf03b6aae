"""Host reference of the grid-fitted immersed boundary (GridFittedBottom, mask_immersed_field!) in numpy, written FROM THE PREDICATE -- a loop
over the cells a node touches, np.where on the whole interior -- and not from count planes, so that it is independent of the kernels'
shortcut; plus the count planes by their definition.

The rule [recalled: Oceananigans' ImmersedBoundaries; its source is not at hand, parity unpinned].  Grid Nz levels, z centres zc[1..Nz]
strictly increasing, h[i, j] the bottom height at (Center, Center) AFTER its halo fill:
  * GridFittedBottom with the centre condition: immersed_cell(i, j, k) = zc[k] <= h[i, j], compared in the grid's float type.  Hence
    c[i, j] = #{k : zc[k] <= h[i, j]} (0 .. Nz) and the immersed cells of a column are k <= c[i, j].
  * inactive_cell = immersed_cell, or k < 1, or k > Nz, or j < 1 where the grid's south side is a wall (serial grid, rank 0 of a band
    chain).  x is periodic: cell i = 0 is read from h's filled west halo column.  Row j = 0 of a band that is not the southernmost is read
    from h's seam halo row.  No node of the interior touches a cell with j > Ny.
  * A node at (LX, LY, LZ) is peripheral if ANY cell it touches is inactive: {i, i-1 if LX is Face} x {j, j-1 if LY is Face} x
    {k, k-1 if LZ is Face}.
  * mask_immersed_field!(field, value) writes value (rounded once to the field's type) to every peripheral node with i = 1..Nx,
    j = 1..Ny, k = 1..Nz of the GRID (a z-Face field's level Nz + 1 is not visited) and touches nothing else.
Arrays are the padded parents, indexed [k + Hz - 1, j + Hy - 1, i + Hx - 1]; locations are 0 (Center) / 1 (Face)."""
import numpy as np


def inactive_cells(h, zc, size, halo, wall):
    """inactive_cell(i, j, k) for i = 0..Nx, j = 0..Ny, k = 0..Nz+1 as a boolean array indexed [k, j, i]; h: padded (Ny+2Hy, Nx+2Hx)
    bottom height, halos filled; zc: the Nz centres, of h's type.  Row j = 0 without a wall needs Hy >= 1, column i = 0 needs Hx >= 1:
    where the halo is missing the cells stay False and mask_immersed_field refuses the locations that would touch them."""
    (Nx, Ny, Nz), (Hx, Hy) = size, halo[:2]
    assert h.dtype == zc.dtype and zc.shape == (Nz,)
    ina = np.zeros((Nz + 2, Ny + 1, Nx + 1), dtype=bool)
    ina[0] = True
    ina[Nz + 1] = True
    j0 = 1 if (wall or Hy < 1) else 0                              # first row / column of cells that h holds
    i0 = 0 if Hx >= 1 else 1
    for k in range(1, Nz + 1):
        ina[k, j0:, i0:] = zc[k - 1] <= h[j0 + Hy - 1:Ny + Hy, i0 + Hx - 1:Nx + Hx]
    if wall:
        ina[:, 0, :] = True
    return ina


def peripheral(ina, loc, size):
    """peripheral_node(i, j, k) for i = 1..Nx, j = 1..Ny, k = 1..Nz, indexed [k-1, j-1, i-1]: any touched cell inactive"""
    Nx, Ny, Nz = size
    xl, yl, zl = loc
    out = np.zeros((Nz, Ny, Nx), dtype=bool)
    for dk in ((0, -1) if zl else (0,)):
        for dj in ((0, -1) if yl else (0,)):
            for di in ((0, -1) if xl else (0,)):
                out |= ina[1 + dk:Nz + 1 + dk, 1 + dj:Ny + 1 + dj, 1 + di:Nx + 1 + di]
    return out


def mask_immersed_field(parent, loc, value, h, zc, size, halo, wall=True, ina=None):
    """the parent after mask_immersed_field!(field, value): ifelse(peripheral, value, c) on i = 1..Nx, j = 1..Ny, k = 1..Nz of the grid.
    `size` is the GRID's; a z-Face field's parent has Nz + 1 levels, the last of which is not visited."""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    assert parent.shape == (Nz + loc[2] + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    if (loc[0] and Hx < 1) or (loc[1] and Hy < 1 and not wall):
        raise ValueError("the node touches a cell that only a halo of h holds")
    per = peripheral(inactive_cells(h, zc, size, halo, wall) if ina is None else ina, loc, size)
    out = parent.copy()
    inner = out[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    inner[...] = np.where(per, parent.dtype.type(value), inner)
    return out, per


def column_counts(h, zc, size, halo, wall):
    """the four count planes by their definition, each (Ny, Nx) int32: c = #{k : zc[k] <= h}, c = Nz for j < 1 behind a wall;
    cc = c, fc = max(c[i], c[i-1]), cf = max(c[j], c[j-1]), ff = max of the four.  A plane whose halo is missing comes back as None."""
    (Nx, Ny, Nz), (Hx, Hy) = size, halo[:2]
    c = np.zeros((Ny + 1, Nx + 1), dtype=np.int32)                 # [j, i] for j = 0..Ny, i = 0..Nx
    for j in range(0, Ny + 1):
        for i in range(0, Nx + 1):
            if (i < 1 and Hx < 1) or (j < 1 and (wall or Hy < 1)):
                continue
            c[j, i] = sum(1 for k in range(Nz) if zc[k] <= h[j + Hy - 1, i + Hx - 1])
    if wall:
        c[0, :] = Nz
    x_ok, y_ok = Hx >= 1, wall or Hy >= 1
    cc = c[1:, 1:].copy()
    fc = np.maximum(c[1:, 1:], c[1:, :-1]) if x_ok else None
    cf = np.maximum(c[1:, 1:], c[:-1, 1:]) if y_ok else None
    ff = np.maximum(np.maximum(c[1:, 1:], c[1:, :-1]), np.maximum(c[:-1, 1:], c[:-1, :-1])) if (x_ok and y_ok) else None
    return {"cc": cc, "fc": fc, "cf": cf, "ff": ff}


def draw_columns(rng, Nx, Ny, Nz):
    """per-column immersed counts c in 0..Nz, (Ny, Nx): in every row columns 0..7 are land (c = Nz), columns 8..15 ocean (c = 0), the
    rest uniform in 0..Nz -- so that at every level chunks of 2 and of 4 columns with no, all and some masked elements occur"""
    c = rng.integers(0, Nz + 1, (Ny, Nx))
    c[:, 0:8] = Nz
    c[:, 8:16] = 0
    return c


def heights_of(c, zc, rng):
    """a bottom height per column whose count is c: exactly the centre zc[c] (1-based: `h equal to a centre is immersed`) for about half
    of the columns, a value strictly between two centres (below the first for c = 0) for the rest; in zc's type"""
    Nz = zc.shape[0]
    lo = np.concatenate([[zc[0] - 1], zc]).astype(zc.dtype)        # lo[c]: the largest height that still gives count c is >= lo[c]
    hi = np.concatenate([zc, [zc[-1] + 1]]).astype(zc.dtype)       # hi[c] > every height of count c
    exact = rng.random(c.shape) < 0.5
    mid = (lo[c].astype(np.float64) + hi[c].astype(np.float64)) / 2
    h = np.where(exact & (c > 0), lo[c], mid.astype(zc.dtype)).astype(zc.dtype)
    got = (zc[:, None, None] <= h[None]).sum(0)
    assert np.array_equal(got, c), "heights_of: a height does not reproduce its count"
    return h


def chunk_classes(n, Nz, W):
    """per level k = 1..Nz of a z-Center field on count plane n: does a W-column chunk with (no, all, some) masked elements occur?"""
    Ny, Nx = n.shape
    m = n[:, :Nx - Nx % W].reshape(Ny, -1, W)
    out = []
    for k in range(1, Nz + 1):
        masked = (k <= m).sum(-1)
        out.append((bool((masked == 0).any()), bool((masked == W).any()), bool(((masked > 0) & (masked < W)).any())))
    return out
