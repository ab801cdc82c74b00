#!/usr/bin/env python3
"""How many tile rows of a map frame does nothing 3D reach?  (profiles/d3_rows/README.md, step 1)

Renders the frame on the CPU oracle and counts the 16-pixel tile rows in which every pixel outside the 2D logo's
box is the 3D miss colour [0, 0, 0, 255].  No GPU.

    python tools/d3_rows_count.py [--width 3840 --height 2160 --lights 16]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TILE = 16


def empty_tile_rows(frame, rect):
    """Indices of the tile rows whose pixels outside [0, rect) x [0, rect) are all the miss colour."""
    h, w, _ = frame.shape
    miss = np.all(frame == np.array([0, 0, 0, 255], np.uint8), axis=2)
    miss[:rect, :rect] = True  # (the logo's box: whatever is drawn there is 2D)
    rows_ok = miss.all(axis=1)
    n_rows = (h + TILE - 1) // TILE
    return [r for r in range(n_rows) if rows_ok[r * TILE:min((r + 1) * TILE, h)].all()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--lights", type=int, default=16)
    ap.add_argument("--rect", type=int, default=200)
    a = ap.parse_args()
    from rusterix_amd import scenes
    from tests.oracle_api import load_oracle

    orc = load_oracle()
    frame = scenes.render(scenes.map_scene(orc, a.width, a.height, n_lights=a.lights, rect_size=float(a.rect)))
    rows = empty_tile_rows(frame, a.rect)
    n_rows = (a.height + TILE - 1) // TILE
    tiles_x = (a.width + TILE - 1) // TILE
    runs = []
    for r in rows:
        if runs and runs[-1][1] == r:
            runs[-1][1] = r + 1
        else:
            runs.append([r, r + 1])
    print(json.dumps(dict(width=a.width, height=a.height, lights=a.lights, tile_rows=n_rows, empty_tile_rows=len(rows),
                          empty_runs=runs, tiles=n_rows * tiles_x, empty_tiles=len(rows) * tiles_x)))


if __name__ == "__main__":
    main()
