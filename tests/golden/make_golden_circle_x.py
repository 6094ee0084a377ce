#!/usr/bin/env python3
"""Generates tests/golden/arm_circle_x.npz from DATA files of the reference checkout (run once where the reference
exists; tests only ever read the .npz written here).  Numbers only: no reference source text is read or stored.

  arm_circle_x.npz    systems/.../simulations/circle_c0-0p7_r0p3_15sec/bilinear_..._2020-06-09_16-43.mat
                      res{1..3}: X (301 x 6, the plant states of the loaded closed loops) and T;
                      ..._2020-06-21_23-31.mat  res_loaded{1..3}: X and W
                      (the fields arm_circle.npz does not hold; together they pin the plant's loaded transitions
                      X(k+1) = Arm.simulate_Ts(X(k), U(k), W(k)), Ksim.m:239-245)
"""
import os

import numpy as np
import scipy.io as sio

REF = '/root/reference'
OUT = os.path.dirname(os.path.abspath(__file__))
BASE = 'systems/thesis-arm-markers_noload_3-mods_1-links_20hz/simulations/circle_c0-0p7_r0p3_15sec/'


def load(rel):
    return sio.loadmat(os.path.join(REF, rel), squeeze_me=False, struct_as_record=False)


def main():
    rc = load(BASE + 'bilinear_poly-3_n-6_m-3_del-0_2020-06-09_16-43.mat')['res']
    rl = load(BASE + 'bilinear_poly-3_n-6_m-3_del-0_2020-06-21_23-31.mat')['res_loaded']
    out = {}
    for i in range(3):
        a = rc[0, i][0, 0]
        out[f'run{i}_X'] = np.asarray(a.X, dtype=np.float64)
        out[f'run{i}_T'] = np.asarray(a.T, dtype=np.float64)
        b = rl[0, i][0, 0]
        out[f'loaded{i}_X'] = np.asarray(b.X, dtype=np.float64)
        out[f'loaded{i}_W'] = np.asarray(b.W, dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, 'arm_circle_x.npz'), **out)


if __name__ == '__main__':
    main()
