"""Inference throughput of the surrogate predictor at the bench codec (factory 'highres': 64 x 64).

For every batch size B (default 1, 32, 288), on one GPU:
  predict            SurrogatePredictor.predict on its static buffers (eval encoder -> head -> gp mean -> ROM),
                     uncaptured launches and the captured HIP graph replay: ms per call, predictions / s;
  encoder forward    the module call encoder(X) in eval mode next to the same module's train-mode forward
                     (batch statistics, Dropout2d draw, running update) with GPI_CONV_SHAPES=0, i.e. both on the
                     generic conv instantiations (the eval launches match no compile-time shape).
The two encoder arms alternate (train block, eval block, ...) inside one process; each block is a host clock
around `--calls` calls ending in a device synchronise; reported: median and min..max over the blocks.

    python tools/infer_bench.py --out profiles/infer_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'generative-physics-informed-pde_amd'))


def block_ms(fn, calls, sync):
    sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    sync()
    return (time.perf_counter() - t0) * 1e3 / calls


def summary(xs):
    return {'median_ms': statistics.median(xs), 'min_ms': min(xs), 'max_ms': max(xs), 'blocks': len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 32, 288])
    ap.add_argument('--calls', type=int, default=200, help='calls per timed block')
    ap.add_argument('--rounds', type=int, default=7, help='timed blocks per arm (arms alternate)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'infer_bench.json'))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('infer_bench needs a GPU: nothing is measured without one')
    from factories.model import ModelFactory
    from gpi.infer import SurrogatePredictor
    from physics.RandomField import NormalRandomFieldSampler
    import numpy as np
    dev = torch.device('cuda:0')
    sync = lambda: torch.cuda.synchronize(dev)
    fac = ModelFactory.FromIdentifier('highres')
    fac.set('device', 'cuda')
    torch.manual_seed(0)
    physics, model, disc, encoder, _, _ = fac.setup()
    disc = disc.to(dev)
    enc = disc._encoder
    n = physics['fom'].grid.n
    rfs = NormalRandomFieldSampler.FromImage(n, n, 0.4, 0.8, 0.04)
    rng = np.random.default_rng(1)
    res = {'config': 'highres', 'imsize': n, 'codec': dict(fac.CODEC), 'drop_rate': enc._cfg['drop_rate'],
           'device': torch.cuda.get_device_name(0), 'calls_per_block': a.calls, 'rounds': a.rounds, 'batches': {}}
    for B in a.batches:
        X = torch.tensor(rfs.sample(batch_size=B, rng=rng), dtype=torch.float32, device=dev).contiguous()
        U = rng.uniform(-0.5, 0.5, (B, 4))
        F = torch.tensor(np.stack([physics['rom'].grid.full_force(u) for u in U]), dtype=torch.float32, device=dev)
        # a few train-mode calls first: running statistics of the data instead of the (0, 1) initial ones
        enc.train()
        os.environ['GPI_CONV_SHAPES'] = '0'
        for _ in range(5):
            enc(X)
        os.environ['GPI_CONV_SHAPES'] = '1'
        enc.eval()
        p = SurrogatePredictor(disc, B)
        y_u = p.predict(X, F).clone()
        p.capture()
        y_c = p.replay().clone()
        assert torch.equal(y_u, y_c), 'captured replay differs from the uncaptured call'
        p.check_flag()

        def train_fwd():
            enc(X)

        def eval_fwd():
            enc(X)

        arms = {'predict_uncaptured': [], 'predict_captured': [], 'encoder_train_generic': [], 'encoder_eval': []}
        for r in range(a.rounds + 1):             # round 0 warms every arm up and is dropped
            enc.train()
            os.environ['GPI_CONV_SHAPES'] = '0'
            t_tr = block_ms(train_fwd, a.calls, sync)
            os.environ['GPI_CONV_SHAPES'] = '1'
            enc.eval()
            t_ev = block_ms(eval_fwd, a.calls, sync)
            t_pu = block_ms(p.predict, a.calls, sync)
            t_pc = block_ms(p.replay, a.calls, sync)
            if r:
                arms['encoder_train_generic'].append(t_tr)
                arms['encoder_eval'].append(t_ev)
                arms['predict_uncaptured'].append(t_pu)
                arms['predict_captured'].append(t_pc)
        out = {k: summary(v) for k, v in arms.items()}
        for k in ('predict_uncaptured', 'predict_captured'):
            out[k]['predictions_per_s'] = B / (out[k]['median_ms'] * 1e-3)
        out['eval_over_train_generic'] = out['encoder_eval']['median_ms'] / out['encoder_train_generic']['median_ms']
        res['batches'][str(B)] = out
        print('B=%d' % B, json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
