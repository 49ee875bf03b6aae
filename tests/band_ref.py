"""One-process emulation of the latitude-band halo fill, written from the protocol's definition: the oracle's passes on
every rank's slab and numpy slicing for the seams -- no device, and nothing of the product (it does not call check_band_widths).

A chain of R bands of widths `sizes` (rank 0 southernmost) over a global (Nx, Ny, Nz) field.  Rank r owns the global rows
j0 + 1 .. j0 + ny (j0 = sum(sizes[:r])); its slab is the padded parent (Nz + 2Hz, ny + 2Hy, Nx + 2Hx).  One fill is
  1. the zipper fold on the last rank only, on that rank's slab with Ny = its own ny;
  2. periodic x on every rank;
  3. ONE seam hop: every rank ships its Hy interior rows next to a seam -- parent rows ny .. ny+Hy-1 northwards, Hy .. 2Hy-1 southwards --
     and writes what it receives into its Hy halo rows on that side.  Every message is taken before any is delivered.
With ny < Hy the "interior rows next to a seam" reach into the band's own halo rows: the slices below take them as they are, which is
what the pack kernel of such a band would ship.
Locations are 0 (Center) / 1 (Face); arrays are indexed [k + Hz - 1, j + Hy - 1, i + Hx - 1]."""
import numpy as np

SENTINEL = 12345.0
LOCATIONS = [(0, 0), (1, 0), (0, 1), (1, 1)]


def default_sign(xl, yl):
    """the zipper sign a Field gets by location: -1 on (Face, Center) / (Center, Face), +1 otherwise"""
    return -1 if xl != yl else 1


def global_field(rng, size, halo, dtype=np.float64):
    """a random padded global field whose y halo rows hold a sentinel (nothing has filled them yet)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    g = rng.uniform(-1, 1, (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)).astype(dtype)
    g[:, :Hy] = SENTINEL
    g[:, Hy + Ny:] = SENTINEL
    return g


def band_rows(sizes, r, Hy):
    """the rows of the padded global parent that rank r's slab covers"""
    j0 = sum(sizes[:r])
    return slice(j0, j0 + sizes[r] + 2 * Hy)


def band_slab(g, sizes, r, Hy):
    """rank r's slab before the fill: its rows of the unfilled global field, its own y halo rows a sentinel"""
    slab = g[:, band_rows(sizes, r, Hy)].copy()
    slab[:, :Hy] = SENTINEL
    slab[:, Hy + sizes[r]:] = SENTINEL
    return np.ascontiguousarray(slab)


def band_fill(oracle, g, sizes, xl, yl, sign, size, halo):
    """the slabs of every rank after one fill of the chain, from the unfilled global field `g` (left unchanged)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    R = len(sizes)
    assert sum(sizes) == Ny and min(sizes) >= 1
    slabs = [band_slab(g, sizes, r, Hy) for r in range(R)]
    oracle.zipper_fill(slabs[-1], xl, yl, sign, (Nx, sizes[-1], Nz), halo)
    for r in range(R):
        oracle.periodic_x_fill(slabs[r], (Nx, sizes[r], Nz), halo)
    north = [s[:, n:n + Hy].copy() for s, n in zip(slabs, sizes)]          # what each rank ships northwards ...
    south = [s[:, Hy:2 * Hy].copy() for s in slabs]                        # ... and southwards
    for r in range(R):
        if r > 0:
            slabs[r][:, :Hy] = north[r - 1]
        if r < R - 1:
            slabs[r][:, Hy + sizes[r]:] = south[r + 1]
    return slabs


def serial_fill(oracle, g, xl, yl, sign, size, halo):
    """the serially filled copy of `g`"""
    return oracle.fill_halo_regions(g.copy(), xl, yl, sign, size, halo)


def differing_cells(slabs, filled, sizes, Hy):
    """number of cells in which the ranks' slabs differ from their rows of the serially filled global field, compared as bits"""
    bits = {8: np.uint64, 4: np.uint32}[filled.dtype.itemsize]
    return sum(int((np.ascontiguousarray(s).view(bits) != np.ascontiguousarray(filled[:, band_rows(sizes, r, Hy)]).view(bits)).sum())
               for r, s in enumerate(slabs))
