"""``model.LibraryModel`` on the GPU: what ``FrozenCLIP`` and ``CustomCLIP`` inherit from it, through one tiny state (embed 128, 7 vision
tokens) and the same calls on both."""
import pytest
import torch

from mudpt_amd import capi
from tests import coop_reference as CR
from tests.test_coop_gpu import build as build_coop
from tests.test_zsclip_gpu import bucket_tokens

pytestmark = pytest.mark.gpu


def test_frozen_and_coop_handles_share_the_base():
    from mudpt_amd.model import LibraryModel, ModelShape
    from mudpt_amd.zsclip import FrozenCLIP
    case = CR.CoopCase("coop_tiny_end")
    B, E = len(case.labels), case.cfg.embed_dim
    assert B == 3
    frozen_shape = ModelShape.from_config(case.cfg, 0, 1)
    handles = {"frozen": FrozenCLIP(frozen_shape, case.frozen, case.tokens, max_batch=B, dtype="fp16"), "coop": build_coop(case, "fp16").eval()}
    for name, m in handles.items():
        assert isinstance(m, LibraryModel)
        with pytest.raises(capi.MudptError, match="no inference forward"):  # the library's bad-state reply to B = 0
            m.image_features()
        logits = m(case.images)
        feats = m.image_features()
        assert tuple(logits.shape) == (B, m.n_cls) and tuple(feats.shape) == (B, E) and feats.dtype == torch.float32, name
        assert torch.equal(m.forward_features(feats), logits), name
        assert torch.equal(m.image_features(), feats), name
        assert torch.equal(m.debug_read("image_features"), feats[0].cpu()), name  # the default batch: one row
        assert torch.equal(m.debug_read("image_features", B).view(B, E), feats.cpu()), name
        m.close()
        m.close()  # harmless
        assert not m._h.value
    # a knob of ``knobs=`` is in place before the weights and the tokens: the text layout is made with it
    tok = bucket_tokens(case.cfg.vocab)  # 2 templates x 96 prompts of two lengths: two buckets by default (tests/test_zsclip_gpu.py)
    for knobs, buckets in ((None, 2), ({"txt_buckets": 1}, 1)):
        m = FrozenCLIP(frozen_shape, case.frozen, tok, max_batch=1, dtype="fp16", knobs=knobs)
        assert m.text_layout()[1] == buckets, knobs
        m.close()
    m = build_coop(case, "fp16", knobs={"txt_buckets": 1})
    assert m.text_layout()[1] == 1
    m.close()
