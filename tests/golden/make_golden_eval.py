"""Eval-mode codec fixtures from the REFERENCE's own torch modules (run where the reference exists,
never on the GPU box):

    python tests/golden/make_golden_eval.py

codec_eval_c32.npz / codec_eval_c64.npz: the codec_c32 / codec_c64 configurations with
drop_rate = 0.2 (eval must switch Dropout2d off), randomised BN affine parameters, running buffers
randomised INDEPENDENTLY per BN layer (mean ~ 0.5 N(0, 1), var in [0.5, 1.5): the BN layers of a dense
block that read the same channels hold different statistics), modules in .eval(), B = 3.
Contents: X, Z, encoder (mu, logsigma), decoder (mean, logsigma), both state dicts, cfg.
The reference is imported the way make_golden.py imports it (FEniCS & co. mocked).
"""
import os

import numpy as np
import torch

from make_golden import CNNEncoder, CNNDecoder, randomize_bn, sd, random_fields, HERE

DROP = 0.2
B = 3


def randomize_running(module, gen):
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(0.5 * torch.randn(m.running_mean.shape, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=gen))
                m.num_batches_tracked.fill_(7)


def make_codec_eval(tag, imsize, dz, latent, blocks, growth, f_enc, f_dec):
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(41)
    enc = CNNEncoder(imsize, dz, blocks, growth, f_enc, drop_rate=DROP)
    dec = CNNDecoder(imsize, dz, (latent, latent), 1, f_dec, blocks, False, growth, drop_rate=DROP,
                     upsample='nearest', force_single_output=False)
    for m in (enc, dec):
        randomize_bn(m, gen)
        randomize_running(m, gen)
        m.eval()
    rng = np.random.default_rng(42)
    X = torch.tensor(random_fields(rng, B, imsize), dtype=torch.float32)
    Z = torch.randn(B, dz, generator=gen)
    with torch.no_grad():
        mu, ls = enc(X)
        mx, lsx = dec(Z)
        mu2, _ = enc(X)
    assert torch.equal(mu, mu2), 'eval-mode reference is not deterministic'
    out = dict(X=X.numpy(), enc_mu=mu.numpy(), enc_ls=ls.numpy(), Z=Z.numpy(), dec_mu=mx.numpy(), dec_ls=lsx.numpy(),
               p=np.float64(DROP), cfg=np.array([imsize, dz, latent, growth, f_enc, f_dec] + list(blocks)))
    out.update(sd(enc, 'enc.'))
    out.update(sd(dec, 'dec.'))
    path = os.path.join(HERE, 'codec_eval_%s.npz' % tag)
    np.savez_compressed(path, **out)
    print('codec eval', tag, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    make_codec_eval('c32', 32, 16, 8, [1, 1], 4, 4, 4)
    make_codec_eval('c64', 64, 64, 8, [1, 2, 1], 4, 6, 6)
