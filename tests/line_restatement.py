"""Plain-Python restatements of the line detector's list processing, shared by test_gpu_line_walk_parallel.py, line_setting_cases.py and
the tests on them: the detector's edge map (the oracle's Canny of the half-resolution image, FastLineDetector's two corners cleared
behind it) and FastLineDetector's seed loop + getPointChain on that map (float32 arithmetic through numpy scalars, so the running mean
of the direction rounds as the oracle's does).  Nothing here needs a GPU."""
import numpy as np

LEN_THR = 20          # FastLineDetector's length_threshold (plv_config default, the oracle's default)
_F = np.float32
_NB = ((1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1))  # {row, col}: getPointChain's neighbour order


def edge_map(lo, eq, low=50, high=50):
    """the detector's edge map: Canny (hysteresis included) of the half-resolution image, then FastLineDetector's two cleared corners"""
    e = lo.canny(lo.resize_half(eq), low, high) != 0
    e[:6, :6] = False
    e[-5:, -5:] = False
    return e


def walk_chains(edges, length_threshold=LEN_THR):
    """lineDetection's seed loop + getPointChain: the kept chains (length_threshold + 1 points or more) in the order of their seeds"""
    h, w = edges.shape
    alive = [list(map(bool, row)) for row in edges]
    chains = []
    for r in range(h):
        row = alive[r]
        for c in range(w):
            if not row[c]:
                continue
            x, y = c, r
            pts = [(x, y)]
            row[c] = False
            direction, step = _F(0), 0
            while True:
                best, best_dir, min_diff = None, 0, _F(7)
                for i, (dr, dc) in enumerate(_NB):
                    ci, ri = x + dc, y + dr
                    if ri < 0 or ri == h or ci < 0 or ci == w or not alive[ri][ci]:
                        continue
                    curr = _F(i - 8 if i > 4 else i)
                    if step == 0:
                        best, direction = (ci, ri), curr
                        break
                    diff = abs(curr - direction)          # float32 - float32 -> float32
                    if diff > _F(4):
                        diff = _F(8) - diff
                    if diff <= min_diff:                  # ties: the later neighbour wins
                        min_diff, best, best_dir = diff, (ci, ri), (i - 8 if i > 4 else i)
                if best is None:
                    break
                if step > 0:
                    if not min_diff < _F(2):
                        break
                    direction = (direction * _F(step) + _F(best_dir)) / _F(step + 1)   # product, sum, quotient: each rounded to float32
                x, y = best
                pts.append(best)
                alive[y][x] = False
                step += 1
            if len(pts) >= length_threshold + 1:
                chains.append(np.array(pts, dtype=np.int32))
    return chains
