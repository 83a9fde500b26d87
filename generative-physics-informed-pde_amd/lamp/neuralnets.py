"""lamp.neuralnets -- the ReLU multilayer perceptron of the reference (lamp/neuralnets.py:7-44).

``FeedforwardNeuralNetwork(dim_in, dim_out, architecture, dropout)`` is an ``nn.Sequential`` named ``layers``
with children ``fc1``, ``activ1``, ..., ``fc{L+1}`` (no activation after the last layer);
``FromLinearDecay`` chooses the L hidden widths on the straight line from dim_in to dim_out, truncated to
integers as the reference does.  The effective-property map (bottleneck/components.py) is its one user here;
its native form is csrc/gpmlp.hip.  Dropout and an output activation are not built."""
import numpy as np
import torch

import lamp.modules


def linear_decay_widths(dim_in, dim_out, num_hidden_layers):
    """Hidden widths of FromLinearDecay: the interior points of linspace(dim_in, dim_out, L + 2), truncated."""
    return [int(w) for w in np.linspace(dim_in, dim_out, num_hidden_layers + 2).astype(int)[1:-1]]


class FeedforwardNeuralNetwork(lamp.modules.BaseModule):

    def __init__(self, dim_in, dim_out, architecture, dropout, outf=None, dtype=None, device=None):
        super().__init__()
        if dropout is not None or outf is not None:
            raise NotImplementedError('FeedforwardNeuralNetwork: dropout / an output activation are not built')
        widths = [int(dim_in)] + [int(w) for w in architecture] + [int(dim_out)]
        self.layers = torch.nn.Sequential()
        for n in range(len(widths) - 1):
            self.layers.add_module('fc%d' % (n + 1), torch.nn.Linear(widths[n], widths[n + 1]))
            if n != len(widths) - 2:
                self.layers.add_module('activ%d' % (n + 1), torch.nn.ReLU())
        self._to(device=device, dtype=dtype)

    @property
    def widths(self):
        """[dim_in, hidden widths ..., dim_out]."""
        fcs = self.linears
        return [fcs[0].in_features] + [fc.out_features for fc in fcs]

    @property
    def linears(self):
        """The nn.Linear layers fc1 .. fc{L+1} in order."""
        return [m for m in self.layers if isinstance(m, torch.nn.Linear)]

    def forward(self, x):
        return self.layers(x)

    @classmethod
    def FromLinearDecay(cls, dim_in, dim_out, num_hidden_layers, outf=None, dropout=None, dtype=None, device=None):
        return cls(dim_in, dim_out, linear_decay_widths(dim_in, dim_out, num_hidden_layers), dropout, outf, dtype,
                   device)
