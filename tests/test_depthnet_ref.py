"""CPU: the fp64 restatement tests/depthnet_ref.py against transformers' DepthAnythingForDepthEstimation in .double() -- this pins the parameter
names, the layer order, the position-embedding interpolation and every resize size before a kernel is compared with the restatement."""
import pytest
import torch

import depthnet_checks as K
import depthnet_ref as R
from aphantasia_amd import depthnet as DN


@pytest.fixture(scope='module')
def hf_model():
    transformers = pytest.importorskip('transformers')
    from transformers import DepthAnythingConfig, DepthAnythingForDepthEstimation, Dinov2Config
    bc = Dinov2Config(hidden_size=128, num_hidden_layers=4, num_attention_heads=2, image_size=518, patch_size=14, out_indices=[1, 2, 3, 4],
                      apply_layernorm=True, reshape_hidden_states=False)
    cfg = DepthAnythingConfig(backbone_config=bc, reassemble_hidden_size=128, neck_hidden_sizes=[16, 32, 64, 64], fusion_hidden_size=32, head_hidden_size=16,
                              reassemble_factors=[4, 2, 1, 0.5])
    torch.manual_seed(0)
    model = DepthAnythingForDepthEstimation(cfg).eval()
    # transformers initialises LayerScale to 1 and biases to 0: seeded values everywhere instead, so that no term can hide
    sd = DN.synthetic_weights(cfg.to_dict(), seed=4, last_bias=0.5)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith('mask_token') for k in missing), (missing, unexpected)
    return cfg.to_dict(), sd, model.double()


@pytest.mark.parametrize('hw', [(56, 84), (126, 182)], ids=lambda s: '%dx%d' % s)
def test_restatement_equals_transformers_fp64(hf_model, hw):
    config, sd, model = hf_model
    img = K.make_image(2, hw[0], hw[1], seed=3)
    with torch.no_grad():
        x = (img.double() - torch.tensor(R.MEAN, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(R.STD, dtype=torch.float64).view(1, 3, 1, 1)
        want = model(pixel_values=x).predicted_depth
        got = R.forward(config, sd, img)
    assert got.shape == want.shape
    assert float((want > 0).double().mean()) > 0.2                 # the last ReLU has not cut the comparison away
    rel = ((got - want).abs().max() / want.abs().max()).item()
    print('restatement vs transformers fp64 %dx%d: max |diff| / max |ref| = %.3e' % (hw[0], hw[1], rel))
    assert rel <= 1e-10


def test_weight_shapes_are_the_state_dict(hf_model):
    config, sd, model = hf_model
    want = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith('mask_token')}
    assert DN.weight_shapes(config) == want


def test_position_rows_identity_and_interpolation():
    pos = torch.randn(1, 1 + 37 * 37, 8)
    assert torch.equal(DN.position_rows(pos, 37, 37), pos[0])
    rows = DN.position_rows(pos, 9, 13)
    assert rows.shape == (1 + 9 * 13, 8) and torch.equal(rows[0], pos[0, 0])
