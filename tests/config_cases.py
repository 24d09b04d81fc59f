"""The small model configurations of the test suites, each stated once and derived from BASE, and the configurations the
model is held to the oracle alone at (tests/test_model_configs_gpu.py, tests/test_page_encoder_cpu.py).  Plain Python: a
test of any kind may import it."""


def make_cfg(roi, hidden, bbox_hidden, use_context=True, addl=0, drop_prob=0.0):
    return dict(roi_output_size=roi, n_classes=4, use_context=use_context, hidden_dim=hidden,
                bbox_hidden_dim=bbox_hidden, n_additional_feat=addl, drop_prob=drop_prob)


def spec_of(cfg):
    """a configuration without drop_prob: the keyword arguments of weights.state_dict_spec / seeded_state_dict"""
    return {k: v for k, v in cfg.items() if k != "drop_prob"}


BASE = make_cfg((3, 3), 32, 8)                      # the smallest head: host-side construction and flat-layout tests
SPLIT_CFG = dict(BASE, drop_prob=0.2)               # the same head with dropout on: trainers stepping over page_set splits
TRAINER_CFG = dict(BASE, hidden_dim=48, bbox_hidden_dim=16)         # trainer_setup's model: the optimizer, loss, SyncBN suites
FEATURE_CFG = dict(TRAINER_CFG, drop_prob=0.3)      # the feature-cache suites: a dropout rate no other suite uses
DDP_CFG = dict(BASE, bbox_hidden_dim=16)            # the gloo data-parallel CPU test
ADDL_SPEC = spec_of(dict(TRAINER_CFG, n_additional_feat=3))         # key-layout tests with additional features
PAGE_SPEC = spec_of(dict(BASE, n_additional_feat=2))                # the page layers' key-layout tests

# ------------------------------------------------------------------------------ configurations held to the oracle only
#          roi     img_h  boxes        cs  hidden  bbox_hidden  seed
ORACLE_CASES = {
    "roi7_T3232": ((7, 7), 96, [33, 20], 12, 64, 32, 211),     # T = 3136 + 32 + 64: the widest ResNet-18 head
    "roi1_ctx": ((1, 1), 64, [14, 9], 2, 64, 16, 212),         # F = 80, T = 144
    "roi4_h384": ((4, 4), 128, [11, 40, 3], 12, 384, 32, 213),  # n_vis = 1024, T = 1440, three pages
}
