"""The 16 x 16 coarse-mesh factories: highres128_rom16 / highres256_rom16 keep the codec of highres128 /
highres256 (so every conv launch keeps its compile-time shape) and change the coarse-grained model only."""
import pytest


@pytest.mark.parametrize('ident,base,n', [('highres128_rom16', 'highres128', 128), ('highres256_rom16', 'highres256', 256)])
def test_rom16_factories(ident, base, n):
    from factories.model import ModelFactory
    fac = ModelFactory.FromIdentifier(ident)
    ref = ModelFactory.FromIdentifier(base)
    assert fac.identifier == ident
    p = fac.params
    assert p['nx_rom'] == p['ny_rom'] == 16
    assert p['nx_rom'] * 2 ** p['num_refines'] == n == ref.params['nx_rom'] * 2 ** ref.params['num_refines']
    phys = fac.physics
    assert phys['fom'].grid.n == n and phys['rom'].grid.n == 16
    W = phys['W']
    assert tuple(W.shape) == ((n + 1) * (n - 1), 17 * 17)         # d_y free fine nodes x coarse nodes
    assert 2 * 16 * 16 == 512                                     # d_x: two triangles per coarse square
    # the codec hyper-parameters (and everything else but the coarse mesh) are the 8 x 8 factory's
    assert type(fac).CODEC == type(ref).CODEC
    rest = lambda q: {k: v for k, v in q.items() if k not in ('nx_rom', 'ny_rom', 'num_refines')}
    assert rest(p) == rest(ref.params)
    # an override still applies
    assert ModelFactory.FromIdentifier(ident, droprate=0.0).params['droprate'] == 0.0


def test_rom16_model_builds():
    """setup() of a 16 x 16 coarse mesh (512 cells: past the reference's cap of 290, which guards its dense
    tensor M) gives a model with d_x = 512; a 17 x 17 mesh is past what gpi_rom solves and is refused."""
    from factories.model import ModelFactory
    fac = ModelFactory.FromIdentifier('highres128_rom16', device='cpu')
    _, model, disc, _, _, _ = fac.setup()
    assert model.g.dim_effective_property == 512 and model.g.dim_out == 16383
    assert tuple(model.gp.fc.weight.shape) == (512, 64)
    from bottleneck.ROM import ROM
    from physics.LinearElliptic import LinearEllipticPhysics
    assert ROM.FromPhysics(LinearEllipticPhysics('rom', 'NDP', 16, refine_to_fom=2)).nc == 16
    with pytest.raises(Exception, match='maximum size'):
        ROM.FromPhysics(LinearEllipticPhysics('rom', 'NDP', 17, refine_to_fom=2))
