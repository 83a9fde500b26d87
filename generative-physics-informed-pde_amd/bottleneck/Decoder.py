"""CNNDecoder (reference bottleneck/Decoder.py:163-325) on the native codec.

Linear latent map -> 1 x 8 x 8 image -> conv0 -> [DenseBlock -> TransitionUp]
-> last decoding -> 2 channels (mean, logsigma), or with ``binary=True`` one
logit channel followed by ``Sigmoid`` (two-phase media, reference
Decoder.py:204-207,240-241).  HomoscedasticCNNDecoder is the reference's
``homoscedastic=True`` variant: one mean channel and a learned log-sigma
plane ``logsigma`` [H, W] shared by every sample (reference
Decoder.py:204-212,271-285); ``ModelFactory(homoscedastic=True)`` builds it.
A plain ``CNNDecoder(homoscedastic=True)`` keeps raising, as it always has
here.  Module tree / order as in the reference; ``forward`` runs the latent
map and the whole conv stack as native kernels.
"""
import torch
import torch.nn as nn

import lamp.modules
from bottleneck.codec import _DenseBlock, _Transition, last_decoding, UnflattenLatentDimension, module_size


class BaseDecoder(lamp.modules.BaseModule):

    @property
    def dim_in(self):
        raise NotImplementedError

    @property
    def dim_out(self):
        raise NotImplementedError

    def propagate_samples(self, Z):
        """Decoder.py:29-37: a sample of the decoder's Gaussian for each z."""
        if getattr(self, '_binary', False):
            raise NotImplementedError('propagate_samples is defined for the Gaussian decoder only')
        means, logsigmas = self.forward(Z)
        if means.shape != logsigmas.shape:
            raise RuntimeError('Implementation assumes that full logsigmas matrix is given; check for broadcasting')
        return means + torch.exp(logsigmas) * torch.randn_like(logsigmas)


class CNNDecoder(BaseDecoder):

    # whether this class builds the homoscedastic head (HomoscedasticCNNDecoder does)
    _builds_homoscedastic = False

    def __init__(self, target_img_size, dim_latent, latent_img_size=(4, 4), latent_img_features=16,
                 init_features=32, blocks=[3, 5, 3], binary=False, growth_rate=8, drop_rate=0., upsample='nearest',
                 force_single_output=False, homoscedastic=False):
        super().__init__()
        if isinstance(target_img_size, tuple):
            assert all(e == target_img_size[0] for e in target_img_size)
            target_img_size = target_img_size[0]
        if isinstance(latent_img_size, tuple):
            assert all(e == latent_img_size[0] for e in latent_img_size)
            latent_img_size = latent_img_size[0]
        out_size = int(latent_img_size * 2 ** len(blocks))
        if out_size != target_img_size:
            raise ValueError('Latent image size {0}x{0} with {1} blocks yields a {2}x{2} output, target is {3}x{3}'
                             .format(latent_img_size, len(blocks), out_size, target_img_size))
        if force_single_output:
            raise NotImplementedError('force_single_output is not supported: the reference then returns a bare mean '
                                      'image, which random_field_likelihood scores as a probability image (the '
                                      'Bernoulli branch), so the variant has no sane ELBO; the native decoder '
                                      'implements the heteroscedastic, homoscedastic and binary heads')
        if homoscedastic and not self._builds_homoscedastic:
            raise NotImplementedError('CNNDecoder implements the heteroscedastic Gaussian head and the binary '
                                      '(Bernoulli) head; the homoscedastic variant (a learned log-sigma plane) is '
                                      'HomoscedasticCNNDecoder, which ModelFactory(homoscedastic=True) builds')
        if upsample != 'nearest':
            raise NotImplementedError('only nearest upsampling is supported')
        self._output_shape = (target_img_size, target_img_size)
        self._dim_in = dim_latent
        self._dim_out = target_img_size ** 2
        self._binary = bool(binary)
        # binary wins over homoscedastic: the reference creates no plane then (Decoder.py:209-210)
        self._homoscedastic = bool(homoscedastic) and not self._binary
        out_channels = 1 if (self._binary or self._homoscedastic) else 2
        if self._homoscedastic:
            # registered before latent_map, as in the reference: state_dict / named_parameters order
            self.logsigma = nn.Parameter(torch.zeros(target_img_size, target_img_size))
        self._latent_img_dimension = latent_img_size ** 2 * latent_img_features
        self._cfg = dict(latent_img_size=latent_img_size, latent_img_features=latent_img_features,
                         init_features=init_features, blocks=list(blocks), growth=growth_rate, out_channels=out_channels,
                         drop_rate=float(drop_rate))
        self.latent_map = nn.Linear(dim_latent, self._latent_img_dimension)
        self.features = nn.Sequential()
        self.features.add_module('unflatten_latent', UnflattenLatentDimension(latent_img_size))
        self.features.add_module('conv0', nn.Conv2d(latent_img_features, init_features, 3, 1, 1, bias=False))
        nf = init_features
        for i, nl in enumerate(blocks):
            self.features.add_module('DecBlock%d' % (i + 1), _DenseBlock(nl, nf, growth_rate, drop_rate))
            nf += nl * growth_rate
            if i < len(blocks) - 1:
                self.features.add_module('TransUp%d' % (i + 1), _Transition(nf, nf // 2, down=False,
                                                                            drop_rate=drop_rate,
                                                                            upsample=upsample))
                nf //= 2
        self.features.add_module('LastTransUp', last_decoding(nf, out_channels, drop_rate=drop_rate,
                                                              upsample=upsample))
        if self._binary:
            self.features.add_module('Sigmoid', nn.Sigmoid())

    def native_config(self):
        return dict(self._cfg)

    @property
    def dim_latent_img(self):
        return self._latent_img_dimension

    @property
    def dim_latent(self):
        return self._dim_in

    @property
    def dim_in(self):
        return self._dim_in

    @property
    def dim_out(self):
        return self._dim_out

    @property
    def model_size(self):
        return module_size(self)

    def forward(self, x, flatten=False):
        from gpi.native import decoder_forward
        out = decoder_forward(self, x)
        if self._binary:
            # the probability image, as the reference's Sigmoid module: the training engine returns the logit
            # image (differentiable), the eval engine the probabilities
            prob = torch.sigmoid(out[:, 0]) if self.training else out[:, 0]
            return prob.reshape(prob.shape[0], -1) if flatten else prob
        if self._homoscedastic:
            # Decoder.py:271-285: the mean image and the plane expanded over the batch (a view: its gradient
            # sums over the samples in autograd)
            mean = out[:, 0]
            logsigmas = self.logsigma.expand((mean.shape[0],) + self._output_shape)
            if flatten:
                return mean.reshape(mean.shape[0], -1), logsigmas.reshape(mean.shape[0], -1)
            return mean, logsigmas
        mean, logsigmas = out[:, 0], out[:, 1]
        if flatten:
            mean = mean.reshape(mean.shape[0], -1)
            logsigmas = logsigmas.reshape(logsigmas.shape[0], -1)
        return mean, logsigmas


class HomoscedasticCNNDecoder(CNNDecoder):
    """The reference's CNNDecoder(homoscedastic=True) (Decoder.py:204-212,271-285): the conv stack ends in one mean
    channel, and ``logsigma`` [H, W] -- the first parameter, registered before ``latent_map`` as in the reference
    -- is the log sigma of every sample.  Same constructor arguments as CNNDecoder; ``binary=True`` wins (the
    reference creates no plane then).  The ELBO engines score it with GPI_EPI_GAUSS_HOMO_LOSS /
    GPI_EPI_GAUSS_HOMO_EXP_LOSS."""

    _builds_homoscedastic = True

    def __init__(self, target_img_size, dim_latent, latent_img_size=(4, 4), latent_img_features=16,
                 init_features=32, blocks=[3, 5, 3], binary=False, growth_rate=8, drop_rate=0., upsample='nearest',
                 force_single_output=False, homoscedastic=True):
        if not homoscedastic:
            raise ValueError('HomoscedasticCNNDecoder is the homoscedastic=True variant; use CNNDecoder otherwise')
        super().__init__(target_img_size, dim_latent, latent_img_size, latent_img_features, init_features, blocks,
                         binary, growth_rate, drop_rate=drop_rate, upsample=upsample,
                         force_single_output=force_single_output, homoscedastic=True)
