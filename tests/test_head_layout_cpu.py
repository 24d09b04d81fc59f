"""weights.head_layout is the one place that adds the widths of the head's context layers up (weights.CONTEXT_LAYERS): for
every option combination of tests/combined_cases.py, with every layer off, with each layer alone and with all four on, its
total is the decoder width of weights.state_dict_spec and CoVA.n_total_feat, and its offsets are the running sum of the
widths in table order behind the F own features."""
import warnings

import pytest

from cova_web_object_detection_amd import weights
from cova_web_object_detection_amd.models import CoVA
import combined_cases as CC

BASE = dict(roi_output_size=(1, 1), n_classes=4, use_context=False, hidden_dim=12, bbox_hidden_dim=7, n_additional_feat=3)
ALONE = {"off": {}, "gat": dict(use_context=True), "readout": dict(page_context_dim=13),
         "page_attn": dict(page_attention_dim=8, page_attention_heads=2, page_attention_geometry=True),
         "page_enc": dict(page_encoder_dim=16, page_encoder_heads=2, page_encoder_layers=2, page_encoder_geometry=True)}
CASES = [("%s-%s" % (w, CC.case_id(row)), CC.build_case(w, row)["cfg"]) for w in CC.WIDTHS for row in CC.matrix()]
CASES += [(name, dict(BASE, **on)) for name, on in ALONE.items()]
CASES += [("all-four", dict(BASE, **{k: v for on in ALONE.values() for k, v in on.items()}))]


@pytest.mark.parametrize("cfg", [c for _, c in CASES], ids=[n for n, _ in CASES])
def test_one_layout_states_the_decoder_width_and_the_offsets(cfg):
    wcfg = {k: v for k, v in cfg.items() if k in weights.SPEC_OPTIONS}
    spec = dict(weights.state_dict_spec(**wcfg))
    n_vis = weights.backbone_channels() * cfg["roi_output_size"][0] * cfg["roi_output_size"][1]
    lay = weights.head_layout(dict(cfg, **weights.page_options(cfg)), n_vis)
    assert (lay.n_vis, lay.Hd, lay.A) == (n_vis, cfg["bbox_hidden_dim"], cfg["n_additional_feat"])
    assert lay.F == n_vis + lay.Hd + lay.A
    assert spec["decoder.1.weight"] == (lay.T, lay.T) and spec["decoder.5.weight"] == (cfg["n_classes"], lay.T)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = CoVA(cfg["roi_output_size"], 64, cfg["n_classes"], **{k: v for k, v in wcfg.items()
                                                                     if k not in ("roi_output_size", "n_classes")})
    assert model.n_total_feat == lay.T and model.n_feat == lay.F
    # table order, a running sum, nothing between the layers; a layer is on exactly when its keys are in the state_dict
    assert [key for key, _, _ in lay.layers] == [layer.key for layer in weights.CONTEXT_LAYERS]
    at = lay.F
    for layer, (_, offset, width) in zip(weights.CONTEXT_LAYERS, lay.layers):
        assert offset == at and width == layer.width(cfg) >= 0
        assert (width > 0) == any(k.startswith(layer.prefix) for k in spec)
        at += width
    assert at == lay.T
    paged = [layer.option for layer, (_, _, w) in zip(weights.CONTEXT_LAYERS, lay.layers) if layer.paged and w > 0]
    assert lay.page_option == (paged[0] if paged else None)
