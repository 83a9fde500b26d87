"""Golden fixture of the optimal effective properties, from the REFERENCE's own function.

Run where the reference checkout exists (see make_golden.py, whose helpers and module mocks this
imports unchanged), never on the GPU box:

    python tests/golden/make_golden_romfit.py

romfit_c32.npz: the reference's OptimizeEffectiveProperties (bottleneck/utils.py:250-282) on the labels and
right-hand sides of rom_c32.npz (nc = 4, r = 8, N = 6), 201 iterations at lr = 1e-2 in fp32 on the CPU, through
the reference's ROM / ReducedOrderModelOperator over the oracle's M and W.  Only the outputs are stored: the
fitted rows, the returned prediction (of iteration 200, before its update), the objective history and the
relative errors logged at iterations 100 and 200.
"""
import os

import numpy as np
import torch

import make_golden as G
from make_golden import R_ROM, R_comp, R_utils

HERE = os.path.dirname(os.path.abspath(__file__))
T, LR = 201, 1e-2


def make_romfit():
    nc, r, mc, mf, M, W, cdofs, fdofs = G.c32_physics()
    d = np.load(os.path.join(HERE, 'rom_c32.npz'))
    rom = R_ROM.ROM(G._Phys(cdofs, fdofs), torch.tensor(M, dtype=torch.float32), torch.float32, 'cpu')
    g = R_comp.ReducedOrderModelOperator(rom, torch.tensor(W, dtype=torch.float32), dtype=torch.float32, device='cpu')
    ds = G._DS(Y=torch.tensor(d['Y']), F_ROM_BC=torch.tensor(d['F']))
    logX, Y_predict, objective, relerr_list = R_utils.OptimizeEffectiveProperties(ds, g, num_iterations=T, lr=LR,
                                                                                   verbose=False)
    np.savez_compressed(os.path.join(HERE, 'romfit_c32.npz'), T=np.int64(T), lr=np.float64(LR),
                        logX=logX.detach().numpy(), Y_predict=Y_predict.detach().numpy(),
                        objective=np.asarray(objective, dtype=np.float64),
                        relerr_list=np.asarray(relerr_list, dtype=np.float64))
    print('romfit ok', objective[0], objective[-1], relerr_list)


if __name__ == '__main__':
    make_romfit()
