"""Text-only path, CPU side: the C ABI's parameter layout against the reference modules' keys, the command line, the refusals."""
import ctypes as C

import pytest
import torch

import smtc_amd  # noqa: F401
from smtc_amd import _lib
import txt_ref as R


def _txt_cfg(**kw):
    base = dict(hidden=768, heads=12, inter=3072, layers=2, vocab=500, max_pos=130, type_vocab=1, txt_kind=_lib.TXT_XLMR, pad_id=1, ln_eps=1e-5,
                num_labels=3, p_hidden=0.1, p_attn=0.1, p_head=0.05, dtype=_lib.BF16, max_posts=4, max_text_len=32, loss_scale=0.0)
    base.update(kw)
    return _lib.TxtConfig(**base)


def _infos(cfg):
    lib, h, out = _lib.lib(), C.c_void_p(), []
    assert lib.mmhip_txt_create(C.byref(cfg), C.byref(h)) == 0
    pi = _lib.ParamInfo()
    for i in range(lib.mmhip_txt_param_count(h)):
        assert lib.mmhip_txt_param_info_at(h, i, C.byref(pi)) == 0
        out.append((pi.name.decode(), tuple(pi.dims[: pi.ndim]), pi.buffer, pi.group, int(pi.offset), int(pi.numel)))
    n, ws = lib.mmhip_txt_numel(h), lib.mmhip_txt_workspace_bytes(h)
    lib.mmhip_txt_destroy(h)
    return out, n, ws


@pytest.mark.parametrize("kind", ["xlmr", "bert"])
def test_layout_is_the_reference_state_dict(kind):
    """names and shapes = the reference modules' state_dict (pooler included); the pooler alone sits in MMHIP_G_NEVER; tensors do not overlap"""
    ocfg = R.oracle_cfg(kind=kind)
    cfg = _txt_cfg(max_pos=ocfg.max_pos, type_vocab=ocfg.type_vocab, txt_kind=_lib.TXT_XLMR if kind == "xlmr" else _lib.TXT_BERT,
                   pad_id=ocfg.pad_id, ln_eps=ocfg.ln_eps_txt)
    infos, numel, ws = _infos(cfg)
    want = R.param_shapes(ocfg)
    assert {n: s for n, s, *_ in infos} == want
    assert want["bert_model.pooler.dense.weight"] == (768, 768) and want["bert_model.pooler.dense.bias"] == (768,)
    for n, _s, buf, grp, _o, _n in infos:
        assert buf == 1
        assert grp == (_lib.G_NEVER if ".pooler." in n else _lib.G_ALWAYS), n
    end = 0
    for _n, _s, _b, _g, off, cnt in sorted(infos, key=lambda x: x[4]):
        assert off >= end and off % 4 == 0
        end = off + cnt
    assert end <= numel
    assert infos[-1][0].endswith("word_embeddings.weight")          # the word table closes the buffer (row-lazy AdamW)
    assert ws > 0


def test_workspace_has_no_image_tower():
    """the text-only carve is smaller than the late-fusion one at the same text shape by at least the image tower's 16-bit weight copies
    (it also drops the tower's activations, the ITM rows and the heads)"""
    lib = _lib.lib()
    _, _, ws_txt = _infos(_txt_cfg())
    mm = _lib.Config(hidden=768, heads=12, inter=3072, layers_txt=2, layers_img=2, vocab=500, max_pos=130, type_vocab=1, txt_kind=1, pad_id=1,
                     ln_eps_txt=1e-5, ln_eps_img=1e-12, image=224, patch=16, proj_dim=512, num_labels=3, fusion=1, p_hidden=0.1, p_attn=0.1,
                     p_head=0.05, dtype=0, max_posts=4, max_text_len=32, loss_scale=0.0)
    h = C.c_void_p()
    assert lib.mmhip_create(C.byref(mm), C.byref(h)) == 0
    ws_mm = lib.mmhip_workspace_bytes(h)
    # a late-fusion handle is not a text-only one, and the other way round
    assert lib.mmhip_txt_param_count(h) == -1 and lib.mmhip_txt_workspace_bytes(h) == 0
    lib.mmhip_destroy(h)
    assert ws_mm - ws_txt >= 2 * (4 * 768 * 768 + 2 * 768 * 3072) * 2


@pytest.mark.parametrize("bad", [dict(num_labels=17), dict(type_vocab=3), dict(max_text_len=129), dict(hidden=704, heads=11), dict(dtype=7)])
def test_create_rejects(bad):
    h = C.c_void_p()
    cfg = _txt_cfg(**bad)
    assert _lib.lib().mmhip_txt_create(C.byref(cfg), C.byref(h)) == -1


def test_parser_accepts_the_reference_command_lines():
    from smtc_amd.run_txt import build_parser, file_names
    p = build_parser()
    a = p.parse_args("--model_name bernice --task 3".split())
    assert (a.epochs, a.weight_decay, a.lr, a.dropout, a.seed) == (2, 0.00025, 1e-5, 0.05, 30)
    assert not (a.testing or a.eval_txt_test or a.save_model or a.save_preds or a.use_loss_correction or a.synthetic) and a.dtype == "bf16"
    a = p.parse_args("--model_name bert --task 2 --epochs 10 --weight_decay 0.01 --lr 2e-5 --dropout 0.1 --seed 7 --testing --eval_txt_test "
                     "--save_model --save_preds --use_loss_correction".split())
    assert a.model_name == "bert" and a.task == 2 and a.epochs == 10 and a.testing and a.save_model and a.save_preds and a.use_loss_correction
    for m in ("bertweet", "roberta"):
        assert p.parse_args(["--model_name", m, "--task", "0"]).model_name == m
    assert p.parse_args("--model_name bernice --task 3 --synthetic --dtype bf16x3".split()).dtype == "bf16x3"
    names = file_names(a, "../results/txt_only/")
    assert names["val"] == "../results/txt_only/bert_task2_seed7_metrics_val.csv" and names["model"].endswith("bert_task2_seed7_net.pth")


def test_refusals():
    from smtc_amd.config import Config
    from smtc_amd.run_txt import build_parser, main
    from smtc_amd.text_only import TextModel
    args = build_parser().parse_args("--model_name bernice --task 3 --synthetic".split())
    cfg = Config(args, multimodal=False, txt=True)
    assert (cfg.num_labels, cfg.batch_size, cfg.max_length) == (3, 16, 128)
    with pytest.raises(NotImplementedError, match="text_only.py:90"):
        TextModel(cfg, "roberta")
    with pytest.raises(NotImplementedError, match="freeze"):
        TextModel(cfg, "bernice", freeze=True)
    with pytest.raises(NotImplementedError, match="use_loss_correction"):
        main("--model_name bernice --task 3 --synthetic --use_loss_correction".split())


def test_world_size_above_one_stops(monkeypatch):
    from smtc_amd.run_txt import main
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="single-process"):
        main("--model_name bernice --task 3 --synthetic".split())


def test_restatement_masks_and_types():
    """the restatement itself: eval logits do not depend on what pad slots hold, token types move them, the pooler gets no gradient"""
    cfg = R.oracle_cfg(kind="bert", hidden=128, heads=2, inter=256, vocab=50, p_hidden=0.0, p_attn=0.0, p_head=0.0)
    P = R.make_params(cfg, 0)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, 50, (2, 8), generator=g)
    mask = torch.ones(2, 8, dtype=torch.int64)
    mask[1, 5:] = 0
    tt = torch.zeros(2, 8, dtype=torch.int64)
    a = R.forward(P, ids, mask, tt, cfg)
    assert torch.allclose(a, R.forward(P, ids, mask, None, cfg), atol=1e-6)
    tt2 = tt.clone()
    tt2[:, 3:] = 1
    assert (R.forward(P, ids, mask, tt2, cfg) - a).abs().max() > 1e-5
    onehot = torch.eye(3, dtype=torch.int64)[[0, 2]]
    _, _, G = R.loss_and_grads(P, ids, mask, tt2, onehot, torch.tensor([1.0, 2.0, 0.5]), cfg)
    assert G["bert_model.pooler.dense.weight"] is None and G["bert_model.embeddings.token_type_embeddings.weight"].abs().min(dim=1).values.min() > 0
