"""fp64 functional restatement of the DenseNet codec in EVAL mode (CPU reference of the inference path).

Follows oracle/codec.py's structure and the reference's parameter names, so that a state_dict drives it
directly; BatchNorm normalises with the layer's running statistics (F.batch_norm(training=False),
eps 1e-5) and Dropout2d is the identity.  Test infrastructure only.
"""
import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-5


def relnorm(a, b):
    """||a - b|| / ||b|| (2-norm over all elements, fp64)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def state64(d, prefix):
    """{name: fp64 tensor} of the floating-point entries 'prefix<name>' of a fixture / state dict."""
    out = {}
    for k, v in d.items():
        if k.startswith(prefix):
            t = torch.as_tensor(np.asarray(v.detach().cpu()) if isinstance(v, torch.Tensor) else np.asarray(v))
            if t.is_floating_point():
                out[k[len(prefix):]] = t.double()
    return out


def _bn_relu(x, p, name):
    return torch.relu(F.batch_norm(x, p[name + '.running_mean'], p[name + '.running_var'], p[name + '.weight'],
                                   p[name + '.bias'], training=False, eps=BN_EPS))


def _conv(x, p, name, stride=1, padding=0):
    return F.conv2d(x, p[name + '.weight'], p.get(name + '.bias'), stride=stride, padding=padding)


def _up(x):
    return F.interpolate(x, scale_factor=2.0, mode='nearest')


def _dense_layer(x, p, name, in_features, growth, bn_size, bottleneck):
    if bottleneck and in_features > bn_size * growth:
        y = _conv(_bn_relu(x, p, name + '.norm1'), p, name + '.conv1')
        y = _conv(_bn_relu(y, p, name + '.norm2'), p, name + '.conv2', padding=1)
    else:
        y = _conv(_bn_relu(x, p, name + '.norm1'), p, name + '.conv1', padding=1)
    return torch.cat([x, y], 1)


def _dense_block(x, p, name, num_layers, in_features, growth, bn_size, bottleneck):
    for i in range(num_layers):
        x = _dense_layer(x, p, '%s.denselayer%d' % (name, i + 1), in_features + i * growth, growth, bn_size,
                         bottleneck)
    return x


def encoder_eval(p, x, imsize, blocks, growth, init_features):
    """CNNEncoder.eval()(x) -> (mean, logsigma)."""
    x = torch.as_tensor(x).double()
    if x.dim() < 4:
        x = x.unsqueeze(1)
    pad = 3 if imsize % 2 == 0 else 2
    h = _conv(x, p, 'features.In_conv', stride=2, padding=pad)
    nf = init_features
    for i, nl in enumerate(blocks):
        h = _dense_block(h, p, 'features.EncBlock%d' % (i + 1), nl, nf, growth, 8, True)
        nf = nf + nl * growth
        t = 'features.TransDown%d' % (i + 1)
        h = _conv(_bn_relu(h, p, t + '.norm1'), p, t + '.conv1')
        h = _conv(_bn_relu(h, p, t + '.norm2'), p, t + '.conv2', stride=2, padding=1)
        nf = nf // 2
    h = h.reshape(h.shape[0], -1)
    h = torch.relu(F.linear(h, p['features.FC.weight'], p['features.FC.bias']))
    mean = F.linear(h, p['features.SplitDense.fc_mean.weight'], p['features.SplitDense.fc_mean.bias'])
    logsig = F.linear(h, p['features.SplitDense.fc_logvar.weight'], p['features.SplitDense.fc_logvar.bias'])
    return mean, logsig


def decoder_eval(p, z, latent_img_size, blocks, growth, init_features):
    """CNNDecoder.eval()(z) -> (mean, logsigma) [B, H, W]."""
    z = torch.as_tensor(z).double()
    h = F.linear(z, p['latent_map.weight'], p['latent_map.bias'])
    h = h.reshape(h.shape[0], -1, latent_img_size, latent_img_size)
    h = _conv(h, p, 'features.conv0', padding=1)
    nf = init_features
    for i, nl in enumerate(blocks):
        h = _dense_block(h, p, 'features.DecBlock%d' % (i + 1), nl, nf, growth, 4, False)
        nf += nl * growth
        if i < len(blocks) - 1:
            t = 'features.TransUp%d' % (i + 1)
            h = _conv(_bn_relu(h, p, t + '.norm1'), p, t + '.conv1')
            h = _conv(_up(_bn_relu(h, p, t + '.norm2')), p, t + '.conv2', padding=1)
            nf = nf // 2
    t = 'features.LastTransUp'
    h = _conv(_bn_relu(h, p, t + '.norm1'), p, t + '.conv1', padding=1)
    h = _conv(_up(_bn_relu(h, p, t + '.norm2')), p, t + '.conv2', padding=1)
    h = _conv(_bn_relu(h, p, t + '.norm3'), p, t + '.conv3', padding=2)
    return h[:, 0], h[:, 1]


def fixture_cfg(d):
    """(imsize, dz, latent, growth, f_enc, f_dec, blocks) of a codec fixture."""
    imsize, dz, latent, growth, f_enc, f_dec = [int(v) for v in d['cfg'][:6]]
    return imsize, dz, latent, growth, f_enc, f_dec, [int(v) for v in d['cfg'][6:]]


def fixture_eval(d):
    """Restatement outputs for a codec_eval fixture: dict enc_mu / enc_ls / dec_mu / dec_ls (fp64 numpy)."""
    imsize, dz, latent, growth, f_enc, f_dec, blocks = fixture_cfg(d)
    mu, ls = encoder_eval(state64(d, 'enc.'), d['X'], imsize, blocks, growth, f_enc)
    mx, lsx = decoder_eval(state64(d, 'dec.'), d['Z'], latent, blocks, growth, f_dec)
    return dict(enc_mu=mu.numpy(), enc_ls=ls.numpy(), dec_mu=mx.numpy(), dec_ls=lsx.numpy())
