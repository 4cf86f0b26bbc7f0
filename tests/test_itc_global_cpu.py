"""CPU: the host side of global-batch ITC -- dist.gather_itc on gloo (world 2 and 3), the new exports of libmmhip.so and their host-side checks
(reservation, capacity, argument rejects: nothing is enqueued on a GPU here), and the --itc_global flag."""
import ctypes as C
import os

import pytest
import torch
import torch.multiprocessing as mp

import smtc_amd  # noqa: F401
from smtc_amd import _lib, build
from smtc_amd import dist as mmdist


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    mmdist.init_from_env(backend="gloo")
    B, E = 3, 8
    # one workspace-like byte buffer per rank, the four tensors are views into it (as MM_Model._gather_itc makes them)
    ws = torch.zeros((2 * B + 2 * world * B) * E * 4, dtype=torch.uint8)
    f = ws.view(torch.float32)
    txt, img = f[:B * E].view(B, E), f[B * E: 2 * B * E].view(B, E)
    txt_all, img_all = f[2 * B * E: (2 + world) * B * E].view(world * B, E), f[(2 + world) * B * E:].view(world * B, E)
    txt.copy_(torch.arange(B * E, dtype=torch.float32).view(B, E) + 1000 * rank)
    img.copy_(-(torch.arange(B * E, dtype=torch.float32).view(B, E) + 1000 * rank))
    mmdist.gather_itc(txt, img, txt_all, img_all)
    want = torch.cat([torch.arange(B * E, dtype=torch.float32).view(B, E) + 1000 * r for r in range(world)])
    ok = torch.equal(txt_all, want) and torch.equal(img_all, -want) and tuple(txt_all.shape) == (world * B, E)
    try:
        mmdist.gather_itc(txt, img, txt_all[:B], img_all)
        ok = False
    except ValueError:
        pass
    q.put((rank, bool(ok)))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gather_itc_rank_order_and_shapes(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29150 + os.getpid() % 300 + world
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got == {r: True for r in range(world)}


def test_gather_itc_without_a_process_group_copies():
    t, i = torch.randn(2, 4), torch.randn(2, 4)
    ta, ia = torch.zeros(2, 4), torch.zeros(2, 4)
    mmdist.gather_itc(t, i, ta, ia)
    assert torch.equal(ta, t) and torch.equal(ia, i)


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.lib()


def _cfg(**kw):
    base = dict(hidden=768, heads=12, inter=3072, layers_txt=2, layers_img=2, vocab=1000, max_pos=130, type_vocab=1, txt_kind=1,
                pad_id=1, ln_eps_txt=1e-5, ln_eps_img=1e-12, image=224, patch=16, proj_dim=512, num_labels=3, fusion=1,
                p_hidden=0.1, p_attn=0.1, p_head=0.05, dtype=0, max_posts=4, max_text_len=64, loss_scale=0.0)
    base.update(kw)
    return _lib.Config(**base)


def test_new_exports_have_signatures(lib):
    for name in ("mmhip_reserve_itc_global", "mmhip_set_itc_global", "mmhip_itc_gather_buffers", "mmhip_op_itc_global_ws_bytes",
                 "mmhip_op_itc_global_fwd", "mmhip_op_itc_global_bwd"):
        assert name in _lib.EXPORTS and getattr(lib, name).argtypes is not None, name
    assert _lib.CB_GATHER_ITC == -4
    assert lib.mmhip_op_itc_global_ws_bytes(512, 64) == ((4 * 16 + 2) * 512 + 2 * 64 * 512 + 2 * 16) * 4
    assert lib.mmhip_op_itc_global_ws_bytes(8193, 1) == 0 and lib.mmhip_op_itc_global_ws_bytes(8, 9) == 0


# mmhip_workspace_bytes of _cfg() / _cfg(dtype=2) handles on the commit before this feature: a handle that never reserves keeps them to the byte
WS_BEFORE = {0: 181023232, 2: 337123840}


@pytest.mark.parametrize("dtype", [0, 2])
def test_reservation_sizes_the_workspace_and_zero_keeps_it(lib, dtype):
    cfg, h = _cfg(dtype=dtype), C.c_void_p()
    assert lib.mmhip_create(C.byref(cfg), C.byref(h)) == 0
    base = lib.mmhip_workspace_bytes(h)
    assert base == WS_BEFORE[dtype]
    assert lib.mmhip_set_itc_global(h, 2, 0) == -3            # nothing reserved
    assert lib.mmhip_set_itc_global(h, 1, 0) == 0
    assert lib.mmhip_reserve_itc_global(h, 0) == 0 and lib.mmhip_workspace_bytes(h) == base
    assert lib.mmhip_reserve_itc_global(h, 1) == 0 and lib.mmhip_workspace_bytes(h) == base
    assert lib.mmhip_reserve_itc_global(h, 4) == 0
    grown = lib.mmhip_workspace_bytes(h)
    G, B, E = 16, 4, 512
    assert grown - base >= (2 * G * E + 2 * B * E) * 4 + lib.mmhip_op_itc_global_ws_bytes(G, B)
    assert grown - base < (2 * G * E + 2 * B * E) * 4 + lib.mmhip_op_itc_global_ws_bytes(G, B) + 16 * 256        # 256-byte rounding of eight slices
    assert lib.mmhip_set_itc_global(h, 4, 3) == 0 and lib.mmhip_set_itc_global(h, 5, 0) == -3
    assert lib.mmhip_set_itc_global(h, 4, 4) == -1 and lib.mmhip_set_itc_global(h, 0, 0) == -1 and lib.mmhip_set_itc_global(h, 2, -1) == -1
    assert lib.mmhip_reserve_itc_global(h, 8192 // 4 + 1) == -1 and lib.mmhip_reserve_itc_global(h, -1) == -1
    assert lib.mmhip_workspace_bytes(h) == grown              # a refused reservation changes nothing
    p = C.c_void_p()
    assert lib.mmhip_itc_gather_buffers(h, C.byref(p), None, None, None) == -2      # not bound
    assert lib.mmhip_reserve_itc_global(h, 0) == 0 and lib.mmhip_workspace_bytes(h) == base
    lib.mmhip_destroy(h)


def test_op_entry_points_reject_on_the_host(lib):
    """no device pointer is dereferenced and nothing is launched for a shape outside the limits"""
    one = C.c_void_p(256)
    f = lib.mmhip_op_itc_global_fwd
    assert f(one, one, one, 8193, 8, None, one, one, one, one, 1 << 40, None) == -1
    assert f(one, one, one, 8, 1025, None, one, one, one, one, 1 << 40, None) == -1
    assert f(one, one, one, 8, 8, None, one, one, one, one, 16, None) == -3
    b = lib.mmhip_op_itc_global_bwd
    assert b(one, one, one, one, one, 16, 8, 9, 8, 1.0, one, one, one, None, None, None, None, one, 1 << 40, None) == -1
    assert b(one, one, one, one, one, 8193, 8, 0, 8, 1.0, one, one, one, None, None, None, None, one, 1 << 40, None) == -1
    assert b(one, one, one, one, one, 16, 8, 0, 1025, 1.0, one, one, one, None, None, None, None, one, 1 << 40, None) == -1
    assert b(one, one, one, one, one, 16, 8, 0, 8, 1.0, one, one, one, None, None, one, None, one, 1 << 40, None) == -1      # d_txt_e without txt_inv


def test_cli_flag_parses_and_is_inert_in_one_process():
    from smtc_amd.run_mm_late import build_parser
    base = ["--txt_model_name", "bernice", "--img_model_name", "vit", "--fusion_name", "attention", "--task", "2"]
    assert build_parser().parse_args(base).itc_global is False
    assert build_parser().parse_args(base + ["--itc_global"]).itc_global is True
    # MMLate_Model hands the option to MM_Model only under data parallelism
    import inspect
    from smtc_amd import mm_late
    assert inspect.signature(mm_late.MM_Model.__init__).parameters["itc_global"].default is False
    seen = {}

    class Probe:
        def __init__(self, *a, **kw):
            seen.update(kw)
            self.device_ = torch.device("cpu")

    import types
    orig = mm_late.MM_Model
    mm_late.MM_Model = Probe
    try:
        cfg = types.SimpleNamespace(batch_size=4, num_labels=3, use_clip_loss=True, beta_itc=0.1, use_tim_loss=False, beta_itm=0.1, max_length=32, dropout=0.0)
        mm_late.MMLate_Model(cfg, "bernice", "vit", "attention", itc_global=True)
    finally:
        mm_late.MM_Model = orig
    assert mmdist.world_size() == 1 and seen["itc_global"] is False
