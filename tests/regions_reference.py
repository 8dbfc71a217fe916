"""The rule of mw_grid_regions (include/mwengine.h, "grid regions") restated without sweeps, labels or atomics: a flood fill from every
unvisited member cell in scan order, Python integers for the representative.  Shares no code with miniworld_amd/csrc/mw_regions.h."""
import numpy as np

NEIGHBOURS = {4: ((-1, 0), (0, -1), (0, 1), (1, 0)),
              8: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def components(member, connectivity):
    """the regions of member != 0 as lists of (j, i), in the order of their lowest flat index (the first cell of each is its root)"""
    gz, gx = np.asarray(member).shape
    m = (np.asarray(member) != 0).tolist()     # (plain lists: the fill indexes cell by cell)
    seen = [[False] * gx for _ in range(gz)]
    steps = NEIGHBOURS[connectivity]
    out = []
    for j0, i0 in ((j, i) for j in range(gz) for i in range(gx)):         # (row-major: scan order)
        if not m[j0][i0] or seen[j0][i0]:
            continue
        seen[j0][i0] = True
        stack, cells = [(int(j0), int(i0))], []
        while stack:
            j, i = stack.pop()
            cells.append((j, i))
            for dj, di in steps:
                nj, ni = j + dj, i + di
                if 0 <= nj < gz and 0 <= ni < gx and m[nj][ni] and not seen[nj][ni]:
                    seen[nj][ni] = True
                    stack.append((nj, ni))
        out.append(cells)
    return out


def representative(cells, gx):
    """the flat index of the cell that minimises (size * j - sum_j)^2 + (size * i - sum_i)^2, ties to the lowest"""
    n = len(cells)
    sj, si = sum(j for j, _ in cells), sum(i for _, i in cells)
    return min(((n * j - sj) ** 2 + (n * i - si) ** 2, j * gx + i) for j, i in cells)[1]


def regions(member, connectivity, min_cells, K, comps=None):
    """(count, size int32[K], cell int32[K], sum int32[K, 2], label int16[gz, gx]) of one env's grid; `comps`: components(member,
    connectivity) where the caller has them already"""
    gz, gx = np.asarray(member).shape
    size, cell, total = np.zeros(K, np.int32), np.full(K, -1, np.int32), np.zeros((K, 2), np.int32)
    label = np.zeros((gz, gx), np.int16)
    count = 0
    for cells in components(member, connectivity) if comps is None else comps:
        code = -1
        if len(cells) >= min_cells:
            if count < K:
                size[count] = len(cells)
                cell[count] = representative(cells, gx)
                total[count] = (sum(j for j, _ in cells), sum(i for _, i in cells))
                code = count + 1
            count += 1
        for j, i in cells:
            label[j, i] = code
    return count, size, cell, total, label


# ---------------------------------------------------------------------------------------------------------------- the shapes
# Legal inputs that take a labelling the most rounds: one region whose cells lie far apart along it.

def serpentine(gz, gx):
    """every other row, joined at alternating ends: one corridor of about gz * gx / 2 cells"""
    m = np.zeros((gz, gx), np.uint8)
    m[0::2] = 1
    for k, j in enumerate(range(1, gz - 1, 2)):
        m[j, gx - 1 if k % 2 == 0 else 0] = 1
    return m


def spiral(gz, gx):
    """a square spiral from the corner inwards, a free cell between its turns"""
    m = np.zeros((gz, gx), np.uint8)
    top, left, bottom, right = 0, 0, gz - 1, gx - 1
    while top <= bottom and left <= right:
        m[top, left:right + 1] = 1
        m[top:bottom + 1, right] = 1
        if bottom - top < 2 or right - left < 2:
            break
        m[bottom, left:right + 1] = 1
        m[top + 2:bottom + 1, left] = 1
        m[top + 2, left + 1] = 1        # (into the next turn)
        top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
    return m


def staircase(gz, gx):
    """steps of one cell down to the left from the top right corner: (k, gx - 1 - k) and (k, gx - 2 - k) — the root is at the far end
    from where row and column sweeps start"""
    m = np.zeros((gz, gx), np.uint8)
    for k in range(min(gz, gx - 1)):
        m[k, gx - 1 - k] = m[k, gx - 2 - k] = 1
    return m


def checkerboard(gz, gx):
    return (np.add.outer(np.arange(gz), np.arange(gx)) % 2 == 0).astype(np.uint8)
