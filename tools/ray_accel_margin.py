#!/usr/bin/env python3
"""The pad constant of the ray box tree (rxr_ray_accel.hip: RXR_RAY_ACCEL_C), measured on the CPU: the smallest power of two C at which
the padded box of a triangle culls no (ray, triangle) pair of tests/ray_accel_ref.py's adversarial generator that Batch3D::intersect's
float32 test accepts.  The library ships 8 x the result.  No device needed.

    tools/ray_accel_margin.py [--seeds 0:12] [--per-kind 250000] [--graze-share 0.5]      # one JSON line
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import ray_accel_ref as A  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", default="0:12")
    ap.add_argument("--per-kind", type=int, default=250000)
    ap.add_argument("--graze-share", type=float, default=0.5)
    a = ap.parse_args()
    lo, hi = (int(x) for x in a.seeds.split(":"))
    C, hits, need = A.measure_C(range(lo, hi), a.per_kind, graze_share=a.graze_share)
    print(json.dumps(dict(seeds=[lo, hi], graze_share=a.graze_share, pairs=(hi - lo) * a.per_kind * len(A.KINDS), accepted_tame_hits=hits, smallest_C=C, per_kind=need,
                          ship=8 * C, shipped_in_header=A.C_SHIPPED, kappa_cap=A.KAPPA_CAP)))


if __name__ == "__main__":
    main()
