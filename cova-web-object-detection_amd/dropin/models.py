"""Drop-in replacement for the reference's ``models.py``: put this directory (and the repo root)
ahead of the reference on PYTHONPATH and ``from models import CoVA`` (reference main.py:10,
evaluate.py:9, extract_attn_wts_and_visualize.py:10) resolves to the MI355X implementation.
``CrossEntropyLoss`` is the criterion of main.py:139 on the same kernels (``from models import CrossEntropyLoss``).
The extensions are defaulted trailing arguments of the same classes (``CoVA(..., attention="gatv2", attention_dropout=0.6)``,
``GraphAttentionLayer(..., attention_dropout=)``, ``CoVA(..., page_context_dim=128)`` with its ``PageReadout`` module,
``CoVA(..., page_attention_dim=128, page_attention_heads=4)`` with its ``PageAttention`` module,
``page_attention_geometry=True`` for the box-geometry bias of its scores, and ``CoVA(..., page_encoder_dim=128,
page_encoder_heads=4, page_encoder_layers=2)`` with its ``PageEncoder`` module, ``page_attention_dropout=`` /
``page_encoder_dropout=`` for the dropout of those two layers): the reference's 9-argument call is
unchanged."""
import cova_amd  # noqa: F401  (registers cova_web_object_detection_amd)
from cova_web_object_detection_amd.models import CoVA, CrossEntropyLoss, GraphAttentionLayer, PageAttention, PageEncoder, PageReadout  # noqa: F401
