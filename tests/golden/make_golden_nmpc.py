#!/usr/bin/env python3
"""Generates tests/golden/arm_nmpc.npz from the reference's stored nonlinear closed loop (numeric data only, as
make_golden.py): systems/thesis-arm-markers_noload_3-mods_1-links_20hz/simulations/blockM_c0p45-0p35_0p5x0p5_15sec/
nonlinear_poly-3_n-6_m-3_del-0_2020-06-13_14-10.mat, res_nonlin: Y, U, R, X, err, comp_time, Z(:, 1:6) and the largest
magnitude of Z(:, 7:end) (the reference pads z with zeros, Kmpc.m:1180)."""
import os

import numpy as np
import scipy.io as sio

REF = '/root/reference'
OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    path = os.path.join(REF, 'systems/thesis-arm-markers_noload_3-mods_1-links_20hz/simulations/blockM_c0p45-0p35_0p5x0p5_15sec/'
                        'nonlinear_poly-3_n-6_m-3_del-0_2020-06-13_14-10.mat')
    r = sio.loadmat(path, squeeze_me=False, struct_as_record=False)['res_nonlin'][0, 0]
    np.savez_compressed(os.path.join(OUT, 'arm_nmpc.npz'), Y=r.Y, U=r.U, R=r.R, X=r.X, err=r.err, comp_time=r.comp_time,
                        Z6=r.Z[:, :6], Zwidth=np.array(r.Z.shape[1]), Zpad_absmax=np.array(np.abs(r.Z[:, 6:]).max()))


if __name__ == '__main__':
    main()
