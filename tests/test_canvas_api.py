"""Per-utterance canvases (lengths and known frames in one batch), host side: the C-ABI additions, AR.canvas_init /
canvas_init_known, the ValueErrors of AR.generate_audio and the slicing of the per-utterance keyword arguments by the
data-parallel layer.  No GPU."""
import datetime
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

NEW_ENTRIES = ("d3pm_denoise_step_canvas", "d3pm_posterior_sample_known", "d3pm_sample_loop_canvas", "d3pm_sample_loop_fp8_canvas")


def test_canvas_entries_are_declared_bound_and_exported(built_lib):
    from vall_e.vall_e import _hip
    header = open(os.path.join(ROOT, "include", "d3pm_hip.h")).read()
    declared = set(re.findall(r"\b(d3pm_[a-z_0-9]+)\s*\(", header))
    for name in NEW_ENTRIES:
        assert name in declared and name in _hip.SIGNATURES and hasattr(built_lib, name), name
    assert re.search(r"typedef struct d3pm_canvas \{[^}]*frame_mask;[^}]*known;[^}]*\} d3pm_canvas;", header, re.S)
    assert built_lib.d3pm_abi_version() == 6
    assert [n for n, _ in _hip.Canvas._fields_] == ["frame_mask", "known"]
    # an entry refuses a null canvas before it touches anything else
    import ctypes as C
    assert built_lib.d3pm_sample_loop_canvas(None, None, 1, None, None, 9, 0, None, None, None, None, 0, 0, 0, None, 0, None, None) == -1
    assert b"null canvas" in built_lib.d3pm_last_error()
    assert C.sizeof(_hip.Canvas) == 2 * C.sizeof(C.c_void_p)


def _native():
    from vall_e.vall_e import AR
    return AR.reference_native()          # parameters on the CPU: canvas_init* stay there too


def test_canvas_init_with_lengths_and_a_known_map():
    from vall_e.vall_e.synth import MASK_ID
    m = _native()
    T = m.cfg.canvas
    assert T == 448
    x, fm = m.canvas_init(3, [3, 448, 1])
    assert x.dtype == torch.int32 and fm.dtype == torch.uint8 and x.shape == (3, T) and fm.shape == (3, T)
    for b, L in enumerate((3, 448, 1)):
        assert x[b].tolist() == [MASK_ID] * L + [0] * (T - L)
        assert fm[b].tolist() == [1] * L + [0] * (T - L)
    # an int keeps today's shared mask
    x1, fm1 = m.canvas_init(2, 5)
    assert fm1.shape == (T,) and fm1.tolist() == [1] * 5 + [0] * (T - 5) and x1[1].tolist() == [MASK_ID] * 5 + [0] * (T - 5)
    x0, fm0 = m.canvas_init(2)
    assert fm0.shape == (T,) and int(fm0.sum()) == m.cfg.n_frames
    # known frames: a prefix (no mask), a scattered map with a known 512 (upstream's mask id doubles as a codec id), nothing
    gap = torch.tensor([7, -1, 512, 9, 1023, 0])
    gm = torch.tensor([True, False, True, False, True, True])
    x, fm, km = m.canvas_init_known(3, [3, 448, 1], known=[torch.tensor([11, 12]), gap, None], known_mask=[None, gm, None])
    assert x[0].tolist() == [11, 12, MASK_ID] + [0] * (T - 3) and km[0].tolist() == [1, 1, 0] + [0] * (T - 3)
    assert x[1].tolist() == [7, MASK_ID, 512, MASK_ID, 1023, 0] + [MASK_ID] * (T - 6)
    assert km[1].tolist() == [1, 0, 1, 0, 1, 1] + [0] * (T - 6)
    assert x[2].tolist() == [MASK_ID] + [0] * (T - 1) and int(km[2].sum()) == 0
    assert fm.sum(dim=1).tolist() == [3, 448, 1] and km.dtype == torch.uint8
    # nothing given at all: no map
    assert m.canvas_init_known(2, 4, known=[None, torch.tensor([3, 4])], known_mask=[None, torch.tensor([False, False])])[2] is None
    # an int n_frames with known frames: per-utterance masks of that length
    x, fm, km = m.canvas_init_known(2, 4, known=[torch.tensor([5]), None])
    assert fm.shape == (2, T) and fm.sum(dim=1).tolist() == [4, 4] and x[0, :5].tolist() == [5, MASK_ID, MASK_ID, MASK_ID, 0]


def test_canvas_init_known_with_levels():
    from vall_e.vall_e import AR
    from vall_e.vall_e.synth import MASK_ID
    m = AR(d_model=32, n_heads=2, num_layers=1, canvas=16, n_frames=8, s_text=4, s_prompt=4, n_q=3)
    ids = torch.tensor([[1, 2, 3], [4, 5, 6]])
    x, fm, km = m.canvas_init_known(1, [5], known=[ids])
    assert x.shape == (1, 16, 3) and x[0, :2].tolist() == ids.tolist() and x[0, 2:5].eq(MASK_ID).all() and x[0, 5:].eq(0).all()
    assert km[0].tolist() == [1, 1] + [0] * 14
    with pytest.raises(ValueError):          # all levels of a known frame are given
        m.canvas_init_known(1, [5], known=[torch.tensor([1, 2])])


_T = [torch.tensor([1, 2, 3])] * 2
_P = [torch.zeros(4, 8, dtype=torch.long)] * 2


@pytest.mark.parametrize("kw", [
    dict(n_frames=[10]),                                                        # wrong list length
    dict(n_frames=[10, 20, 30]),
    dict(n_frames=[10, 20], known=[torch.tensor([1])]),
    dict(n_frames=[10, 20], known=[None, None], known_mask=[None]),
    dict(n_frames=[0, 20]),                                                     # L_b outside 1 .. canvas
    dict(n_frames=[10, 449]),
    dict(n_frames=[10, 20], known=[torch.tensor([1, 1024]), None]),             # id outside 0 .. 1023
    dict(n_frames=[10, 20], known=[None, torch.tensor([-1])]),
    dict(n_frames=[10, 20], known=[torch.arange(11), None]),                    # a known frame at or beyond L_b
    dict(n_frames=[10, 20], known=[torch.zeros(30, dtype=torch.long), None],
         known_mask=[torch.arange(30) == 10, None]),
    dict(n_frames=10, known=[torch.arange(11), None]),
    dict(known=[torch.zeros(351, dtype=torch.long), None]),                      # the constructor's n_frames = 350
    dict(n_frames=[10, 20], known=[torch.tensor([1, 2]), None], known_mask=[torch.tensor([True]), None]),   # mask / ids lengths differ
    dict(n_frames=[10, 20], known_mask=[None, None]),                           # a mask without ids
    dict(n_frames=[10, 20], known=[torch.tensor([0.5]), None]),                 # not integer ids
    dict(n_frames=[10, 20], graph=True),                                        # the graph path never ignores the arguments
    dict(known=[torch.tensor([1]), None], graph=True),
])
def test_generate_audio_rejects_bad_per_utterance_arguments_on_the_host(kw):
    """ValueError before anything touches the GPU: the model lives on the CPU here, and a valid call would raise the
    RuntimeError of a missing HIP device instead."""
    with pytest.raises(ValueError):
        _native().generate_audio(_T, _P, **kw)


def test_valid_per_utterance_arguments_reach_the_device_check():
    m = _native()
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.generate_audio(_T, _P, n_frames=[10, 448], known=[torch.tensor([1, 512]), None])
    with pytest.raises(RuntimeError, match="no CPU path"):      # an in-range gap map whose unmarked entries are placeholders
        m.generate_audio(_T, _P, n_frames=[3, 20], known=[torch.tensor([5, -7, 9]), None], known_mask=[torch.tensor([True, False, True]), None])


# ---- data-parallel slicing over gloo -----------------------------------------------------------------------------------------
CANVAS = 16


class _FakeModel:
    class cfg:
        canvas, n_frames = CANVAS, 12
    device = torch.device("cpu")


class _FakeNAR:
    n_resp_levels, n_tokens = 7, 1024


def _args(n_utts):
    lens = [1 + (5 * i) % CANVAS for i in range(n_utts)]
    known = [None if i % 3 == 0 else torch.arange(min(lens[i], 1 + i % 4)) + 10 * i for i in range(n_utts)]
    kmask = [None if k is None or i % 2 else torch.arange(k.shape[0]) % 2 == 0 for i, k in enumerate(known)]
    return lens, known, kmask


def _recording_generate(log):
    def fn(texts, proms, *, seed, utt0, n_frames, known, known_mask):
        log.append((utt0, list(n_frames), known, known_mask))
        assert len(texts) == len(n_frames) == len(known) == len(known_mask)
        rows = []
        for b, t in enumerate(texts):
            g = torch.Generator().manual_seed(seed * 1000 + utt0 + b)
            row = torch.randint(0, 1024, (CANVAS,), generator=g) + int(t[0])
            if known[b] is not None:
                given = torch.ones(known[b].shape[0], dtype=torch.bool) if known_mask[b] is None else known_mask[b]
                row[: known[b].shape[0]][given] = known[b][given]
            rows.append(row)
        return torch.stack(rows) if len(rows) > 1 else rows[0]
    return fn


def _fake_nar(texts, proms, resps, *, seed, utt0):
    out = []
    for b, r in enumerate(resps):
        g = torch.Generator().manual_seed(seed * 7919 + utt0 + b)
        out.append(torch.cat([r.long(), torch.randint(0, 1024, (r.shape[0], 7), generator=g)], dim=-1))
    return out


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


def _run(dp, n_utts, rank, world):
    texts = [torch.tensor([i]) for i in range(n_utts)]
    lens, known, kmask = _args(n_utts)
    log = []
    grid = dp.generate_audio_dp(_FakeModel(), texts, texts, seed=3, generate_fn=_recording_generate(log), n_frames=lens, known=known,
                                known_mask=kmask)
    lo, hi = dp.shard_bounds(n_utts, world, rank)
    if hi > lo:       # this rank received exactly its slice of every per-utterance argument
        (utt0, got_lens, got_known, got_mask), = log
        assert utt0 == lo and got_lens == lens[lo:hi]
        assert all(_same(a, b) for a, b in zip(got_known, known[lo:hi])) and all(_same(a, b) for a, b in zip(got_mask, kmask[lo:hi]))
    else:
        assert not log
    log2 = []
    codes = dp.generate_codes_dp(_FakeModel(), _FakeNAR(), texts, texts, seed=3, ar_fn=_recording_generate(log2), nar_fn=_fake_nar,
                                 n_frames=lens, known=known, known_mask=kmask)
    assert (not log2) if hi == lo else (log2[0][0] == lo and log2[0][1] == lens[lo:hi])
    return grid, codes


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n_utts, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from vall_e.vall_e import dp
    q.put((rank,) + _run(dp, n_utts, rank, world))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_utts", [(2, 5), (3, 4), (3, 2)])
def test_dp_slices_per_utterance_arguments_and_gathers_the_world_1_grid(world, n_utts):
    from vall_e.vall_e import dp
    single, single_codes = _run(dp, n_utts, 0, 1)
    lens, known, kmask = _args(n_utts)
    assert single.shape == (n_utts, CANVAS)
    assert single_codes.shape == (n_utts, max(lens), 8) and single_codes.dtype == torch.int64
    for b, L in enumerate(lens):       # the NAR stage saw utterance b's own L_b frames; zero beyond them
        assert torch.equal(single_codes[b, :L, 0], single[b, :L].clamp(max=1023)) and single_codes[b, L:].eq(0).all()
        assert single_codes[b, :L, 1:].any()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_utts, q), daemon=True) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r for r, _, _ in got) == list(range(world))
    for r, grid, codes in got:
        assert torch.equal(grid, single), r
        assert torch.equal(codes, single_codes), r
