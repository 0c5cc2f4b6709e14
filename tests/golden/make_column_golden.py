#!/usr/bin/env python3
"""Golden vectors for the graph module's columns (glv_batch_set_column_texels), produced by evaluating the reference's SHADER TEXT of
smooth_audio_adj (shaders/glava/util/smooth.glsl:67-73) with _PRE_SMOOTHED_AUDIO 1 -- three texelFetch results added and divided by
3.0F -- through tests/glsl_eval.py, at the positions graph/1.frag:87-88 passes: idx / half_w and pixel = 1.0F / float(screen.x).

A column whose table (glava_amd.bar_positions.graph_column_texels) has a tie or a `beyond` entry is left out (stored as NaN; its fetch is
undefined in GLSL or its rounding direction is the implementation's): tests/test_column_texels_host.py states how many.

Needs the reference tree (run in the build container); writes tests/golden/column_vectors.npz, which travels to the GPU box.  The texel
rows are regenerated from the seeds below by the tests.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import glsl_eval as G  # noqa: E402
from glava_amd.bar_positions import graph_column_texels  # noqa: E402

F = np.float32
CASES = [(1024, 320, 31), (1024, 801, 32), (4096, 510, 33), (4096, 800, 34), (4096, 1920, 35), (16384, 801, 36), (16384, 1280, 37)]   # n, screen width, seed


def texel_row(n, seed):
    """a spectrum-like row of GL_R16 texels"""
    rng = np.random.default_rng(seed)
    x = rng.random(n) ** 3 * 1.3 - 0.1
    return np.rint(np.clip(x, 0, 1) * 65535).astype(np.uint16)


def texel_floats(c):
    """what texelFetch returns for GL_R16 texels c: c / 65535, correctly rounded"""
    return (c.astype(F) / F(65535)).astype(F)


def evaluate(n, screen_w, seed):
    sh = G.load("util/smooth.glsl", {"_SMOOTH_FACTOR": repr(0.025), "_PRE_SMOOTHED_AUDIO": 1})
    tex = G._Tex(texel_floats(texel_row(n, seed)))
    _, ties, beyond = graph_column_texels(n, screen_w)
    half_w = F(screen_w // 2)
    pixel = F(F(1.0) / F(screen_w))
    out = np.full(len(ties), np.nan, F)
    for i in range(len(ties)):
        if ties[i].any() or beyond[i].any():
            continue
        out[i] = sh.call("smooth_audio_adj", tex, n, F(F(i) / half_w), pixel)
    return out


def main():
    out = {f"graph_n{n}_w{w}_s{seed}": evaluate(n, w, seed) for n, w, seed in CASES}
    np.savez_compressed(os.path.join(HERE, "column_vectors.npz"), **out)
    print("wrote", len(out), "vectors")


if __name__ == "__main__":
    main()
