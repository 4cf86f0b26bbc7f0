"""CPU: the host side of global-norm gradient clipping (max_grad_norm) -- the command-line flag, the default that builds nothing and calls nothing
new, the calls an armed trainer makes (a recording stand-in for the library), the per-epoch log line, the refusal under data parallelism, and the
C ABI's exports."""
import importlib
import types

import pytest
import torch

import smtc_amd  # noqa: F401
from smtc_amd import _lib, engine_module
from smtc_amd import dist as mmdist
from test_one_tower_cpu import STDOUT, _bare, _run_epochs, _text_batches

NEW_EXPORTS = {"mmhip_grad_clip_state_bytes", "mmhip_set_grad_clip", "mmhip_txt_set_grad_clip", "mmhip_img_set_grad_clip", "mmhip_op_grad_clip",
               "mmhip_adamw_clipped", "mmhip_adamw_rows_clipped"}
STATE_BYTES = 16 + 4 * 1024


@pytest.mark.parametrize("module,sample", [("run_mm_late", ["--txt_model_name", "bernice", "--img_model_name", "vit", "--fusion_name", "attention", "--task", "2"]),
                                           ("run_txt", ["--model_name", "bernice", "--task", "3"]), ("run_img", ["--model_name", "vit", "--task", "3"])])
def test_the_flag_parses_and_is_documented(module, sample):
    mod = importlib.import_module("smtc_amd." + module)
    p = mod.build_parser()
    assert p.parse_args(sample).max_grad_norm is None                                   # default: off
    assert p.parse_args(sample + ["--max_grad_norm", "1.0"]).max_grad_norm == 1.0
    with pytest.raises(SystemExit):
        p.parse_args(sample + ["--max_grad_norm", "much"])
    assert "--max_grad_norm" in mod.__doc__.split("Additive flags")[1].split("\n\n")[0]


def test_the_early_fusion_command_line_has_no_such_flag():
    from smtc_amd import run_mm_early
    assert "max_grad_norm" not in run_mm_early.__doc__ and not any("--max_grad_norm" in a.option_strings for a in run_mm_early.build_parser()._actions)


def test_the_exports_are_declared():
    assert NEW_EXPORTS <= set(_lib.EXPORTS)
    hdr = open(__file__.replace("tests/test_gradclip_cpu.py", "include/mmhip.h")).read()
    for name in NEW_EXPORTS:
        assert name + "(" in hdr, name


class _Recorder:
    """stands in for the loaded library: every entry point answers 0 (the state size: its bytes) and is written down"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return STATE_BYTES if name == "mmhip_grad_clip_state_bytes" else 0
        return fn


def _trainer(monkeypatch, word=False):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    m = object.__new__(engine_module.WordTableEngineModule if word else engine_module.GuardedEngineModule)
    torch.nn.Module.__init__(m)
    m.device_, m._handle, m.backward_products = torch.device("cpu"), 123, None
    m._flat_train, m._flat_grad = torch.zeros(64), torch.zeros(64)
    m._nonfinite = torch.zeros(2, dtype=torch.int32)
    if word:
        m._word_info = dict(offset=32, shape=(4, 8), numel=32)
        m._word_row_state = torch.zeros(4, dtype=torch.uint8)
    t = object.__new__(engine_module.FlatTrainer)
    t.model, t._opt, t.device = m, None, torch.device("cpu")
    return t, rec


@pytest.mark.parametrize("word", [False, True])
def test_the_default_builds_no_state_and_calls_no_new_entry_point(monkeypatch, capsys, word):
    t, rec = _trainer(monkeypatch, word)
    t.set_max_grad_norm(None)
    t._grad_clip_norm([(0, 64)], 1.0)
    t._adamw_ranges([(0, 64)], 1e-3, 0.01, 1, 1.0)
    t.model._apply_setters(t.model._handle) if not word else None
    t._log_grad_clip()
    names = [n for n, _ in rec.calls]
    assert names == ["mmhip_adamw_guarded"] + (["mmhip_adamw_rows_guarded"] if word else ["mmhip_set_guard"])
    assert not NEW_EXPORTS & set(names) and t.model._grad_clip is None and t.max_grad_norm is None and t.grad_clip_stats() is None
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("word", [False, True])
def test_an_armed_trainer_takes_the_norm_and_then_the_clipped_forms(monkeypatch, word):
    t, rec = _trainer(monkeypatch, word)
    t.set_max_grad_norm(0.5)
    max_norm, state = t.model._grad_clip
    assert max_norm == 0.5 and state.numel() == STATE_BYTES and state.dtype == torch.uint8 and not bool(state.any())
    assert [n for n, _ in rec.calls] == ["mmhip_grad_clip_state_bytes", "mmhip_set_grad_clip"]
    assert rec.calls[1][1][0] == 123 and rec.calls[1][1][1] == 0.5 and rec.calls[1][1][2].value == state.data_ptr()
    del rec.calls[:]
    t._grad_clip_norm([(0, 8), (16, 64)], 0.5)
    t._adamw_ranges([(0, 8), (16, 64)], 1e-3, 0.01, 1, 0.5)
    names = [n for n, _ in rec.calls]
    assert names == ["mmhip_op_grad_clip", "mmhip_adamw_clipped", "mmhip_adamw_clipped"] + (["mmhip_adamw_rows_clipped"] if word else [])
    seg_g, seg_n, segments, row_g, rows, width, row_state, mx, gs, guard, st, _ = rec.calls[0][1]
    g0 = t.model._flat_grad.data_ptr()
    ends = (8, 32) if word else (8, 64)
    assert segments == 2 and list(seg_g[:2]) == [g0, g0 + 64] and list(seg_n[:2]) == [ends[0], ends[1] - 16] and (mx, gs) == (0.5, 0.5)
    assert st.value == state.data_ptr() and guard.value == t.model._nonfinite.data_ptr()
    assert (rows, width, row_g.value, row_state.value) == (4, 8, g0 + 128, t.model._word_row_state.data_ptr()) if word else (rows == 0 and row_g is None and row_state is None)
    for _, args in rec.calls[1:]:
        assert args[-1].value == state.data_ptr() and args[-2].value == t.model._nonfinite.data_ptr()
    # a re-created handle is armed again; a second arming keeps the block (and its counters); None disarms on the handle
    del rec.calls[:]
    t.model._apply_setters(456) if not word else None
    t.set_max_grad_norm(2.0)
    assert t.model._grad_clip[1] is state and rec.calls[-1][0] == "mmhip_set_grad_clip" and rec.calls[-1][1][1] == 2.0
    if not word:
        assert ("mmhip_set_grad_clip", 456) in [(n, a[0]) for n, a in rec.calls]
    t.set_max_grad_norm(None)
    assert t.model._grad_clip is None and rec.calls[-1][0] == "mmhip_set_grad_clip" and rec.calls[-1][1][1:] == (0.0, None)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            t.set_max_grad_norm(bad)


def test_train_logs_one_line_per_epoch_only_when_armed(monkeypatch, tmp_path, capsys):
    from smtc_amd.text_only import TextModel
    words = torch.zeros(STATE_BYTES, dtype=torch.uint8)
    words[:16].view(torch.float32)[:2] = torch.tensor([0.25, 4.0])
    words[:16].view(torch.int32)[2:] = torch.tensor([5, 9], dtype=torch.int32)
    tr = _bare(TextModel, with_types=True, max_grad_norm=1.0)
    tr.model._grad_clip = (1.0, words)
    assert tr.grad_clip_stats() == dict(norm=4.0, coef=0.25, clipped_steps=5, steps=9)
    _, _, out, _, _ = _run_epochs(tr, _text_batches(), monkeypatch, tmp_path, capsys)
    line = "grad clip (max_grad_norm 1): last norm 4 coef 0.25, clipped 5 of 9 steps\n"
    assert out == "".join(chunk + "test\n" + line for chunk in STDOUT.split("test\n")[:-1])


@pytest.mark.parametrize("which", ["late", "txt", "img"])
def test_world_size_above_one_raises_and_says_why(monkeypatch, which):
    monkeypatch.setattr(mmdist, "world_size", lambda: 2)
    cfg = types.SimpleNamespace(batch_size=4, num_labels=3, use_clip_loss=False, beta_itc=0.1, use_tim_loss=False, beta_itm=0.1, max_length=32, dropout=0.0)
    with pytest.raises(NotImplementedError) as e:
        if which == "late":
            from smtc_amd.mm_late import MMLate_Model
            MMLate_Model(cfg, "bernice", "vit", "attention", max_grad_norm=1.0)
        elif which == "txt":
            from smtc_amd.text_only import TextModel
            TextModel(cfg, "bernice", max_grad_norm=1.0)
        else:
            from smtc_amd.image_only import ImageModel
            ImageModel(4, 3, "vit", max_grad_norm=1.0)
    msg = str(e.value)
    assert "max_grad_norm" in msg and "word-table rows arrive after the dense optimizer" in msg and "sum of partial norms across ranks" in msg
