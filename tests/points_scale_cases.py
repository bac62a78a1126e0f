"""Shared cases of the one-scalar point multiplication tests (tests/test_points_scale_host.py on a CPU,
tests/test_gpu_points_scale.py on the GPU): the scalar list of the issue and dg16_points_mul's rows of DESIGN.md 2.9."""

import random

from oracle.pyref.fields import FR

# (doublings, additions) per product of dg16_points_mul, table included, by the number of parts
POINTS_MUL_ROW = {1: (256, 67), 2: (128, 67), 4: (68, 71)}
N_RANDOM = 64


def fixed_scalars(curve, w):
    r = FR[curve].p
    return [0, 1, 2, 3, (1 << w) - 1, 1 << w, r - 2, r - 1, r, r + 1, (1 << 255) - 1, int("1" * 64, 16), int("5" * 64, 16)]


def random_scalars(curve, seed=2024):
    """half below r, half below 2^255 (a canonical input may hold either)"""
    rng = random.Random(seed)
    r = FR[curve].p
    return [rng.randrange(r) for _ in range(N_RANDOM // 2)] + [rng.randrange(1 << 255) for _ in range(N_RANDOM // 2)]


def scalar_list(curve, w):
    return fixed_scalars(curve, w) + random_scalars(curve)
