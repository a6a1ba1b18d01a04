"""CPU: the host side of batched alignment - the symbols and their argument checks that answer before any HIP call, the ranking
of best-of-N by alignment on hand-made values, and the argument checks of VALLE.align_batch.  What needs an engine runs in
test_gpu_align_batch.py."""
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


def test_align_batch_symbols_exist_and_refuse_bad_arguments_without_gpu(lib):
    import ctypes as C

    from valle_amd import engine

    for name in ("vx_align_batch", "vx_op_attn_text_segs", "vx_op_mono_path_segs"):
        assert hasattr(lib, name) and name in engine.declared_symbols()
    assert lib.vx_align_batch(None, 1, *([None] * 13)) == 1 and b"null" in lib.vx_last_error()
    assert lib.vx_op_mono_path_segs(None, 1, None, None, None, None) == 1 and b"null" in lib.vx_last_error()
    wide = (C.c_int64 * 4)(5000, 5000, 0, 0)
    assert lib.vx_op_mono_path_segs(8, 1, wide, 8, 8, None) == 4 and b"4096" in lib.vx_last_error()  # refused before any HIP call
    # (start, text_len, qfirst, rows, row0, c0, c1, cell_off, row_off): a start off the 64-row grid, a window past the text, cells
    # past the output
    for desc, match in (((32, 7, 9, 4, 2, 0, 7, 0, 0), b"multiple of 64"), ((64, 7, 9, 4, 2, 2, 9, 0, 0), b"window"),
                        ((64, 7, 9, 4, 2, 0, 7, 1, 0), b"outside the outputs")):
        assert lib.vx_op_attn_text_segs(8, 8, 192, 1, (C.c_int64 * 9)(*desc), 1, 8, 8, None, 28, 4, 1, None) == 1
        assert match in lib.vx_last_error(), lib.vx_last_error()


def _alignment(T, Sw, path_score, path=True):
    from valle_amd.models import Alignment

    p = torch.zeros(T, dtype=torch.int32) if path else None
    return Alignment(torch.zeros(T, Sw), torch.zeros(T), p, path_score if path else float("-inf"), None, None, torch.zeros(Sw))


def _glp(mean, n=4):
    from valle_amd.models import GenLogProbs

    return GenLogProbs(torch.full((n,), float(mean)), None, n, 3)  # a length stop: ar_mean is the mean of the n terms


def test_alignment_rank_key():
    from valle_amd.models import alignment_rank_key

    assert alignment_rank_key(_alignment(10, 3, -25.0)) == -2.5                      # path_score / T
    assert alignment_rank_key(_alignment(2, 3, 0.0, path=False)) == float("-inf")    # T < Sw: no path
    assert alignment_rank_key(None) == float("-inf")                                 # an empty output
    assert alignment_rank_key(_alignment(10, 3, -25.0), _glp(-1.0)) == -2.5          # the log-probabilities do not enter


def test_best_of_rank_order_and_tie_rules():
    from valle_amd.models import alignment_rank_key, best_of_index, best_of_rank

    inf = float("inf")
    als = [_alignment(10, 3, -30.0), _alignment(20, 3, -40.0), None, _alignment(2, 3, 0.0, path=False)]
    means = [_glp(v).ar_mean for v in (-1.0, -3.0, -0.5, -0.25)]
    keys = [alignment_rank_key(a, None) for a in als]
    assert keys == [-3.0, -2.0, -inf, -inf]
    assert best_of_rank(keys, means) == 1                       # the highest key; neither the best mean nor the longest output
    assert best_of_rank([-2.0, -2.0, -3.0], [-1.0, -0.5, -0.1]) == 1  # a tie goes to the higher ar_mean
    assert best_of_rank([-2.0, -2.0, -3.0], [-0.5, -0.5, -0.1]) == 0  # then to the lower index
    assert best_of_rank([-inf, -5.0, -inf], [-0.1, -9.0, -0.2]) == 1  # no path ranks last whatever its mean
    assert best_of_rank([float("nan"), -5.0], [-0.1, -9.0]) == 1      # so does a key that is not a number
    assert best_of_rank([-2.0, -2.0], [float("nan"), -7.0]) == 1      # an ar_mean of NaN (nothing emitted) loses the tie
    no_path = [-inf, -inf, -inf]
    for means3 in ([-1.0, -0.5, -0.7], [-0.5, -0.5, -0.7], [float("nan"), -2.0, -2.0]):
        assert best_of_rank(no_path, means3) == best_of_index(means3)  # nobody has a path: the log-probability's order
    with pytest.raises(ValueError):
        best_of_rank([-1.0], [-1.0, -2.0])
    with pytest.raises(ValueError):
        best_of_rank([], [])


def test_best_of_carries_alignments_and_keys():
    from valle_amd.models import BestOf

    b = BestOf(0, [1], [-1.0], [torch.zeros(3)])
    assert b.alignments is None and b.rank_key is None and b.logprobs is None  # the fields of the earlier form still construct


@pytest.mark.parametrize("cls", ["VALLE", "VALLF"])
def test_align_batch_argument_checks_before_any_engine(cls):
    """As test_align_argument_checks_before_any_engine: every check of every utterance answers with ValueError on a model that
    has no device; with valid arguments the engine is what is missing."""
    from valle_amd import models

    m = getattr(models, cls)(128, 2, 2).eval()
    x, x_lens = torch.randint(3, 50, (1, 6)), torch.tensor([6])
    y = torch.randint(0, 1024, (1, 10, 8))
    u = (x, x_lens, y)
    assert m.align_batch([], 3) == []
    with pytest.raises(ValueError, match="2 prompt_frames for 3 utterances"):
        m.align_batch([u, u, u], [3, 3])
    with pytest.raises(ValueError, match="head"):
        m.align_batch([u], 3, heads=[(0, 2)])
    with pytest.raises(ValueError, match="heads"):
        m.align_batch([u], 3, heads=torch.zeros(2, 2))
    with pytest.raises(ValueError, match="window"):
        m.align_batch([u, (x, x_lens, y, torch.tensor([6]))], 3)
    with pytest.raises(ValueError, match="prepend_bos"):
        m.align_batch([u, u], [3, 0])
    with pytest.raises(ValueError, match="prompt_frames"):
        m.align_batch([u, u], [10, 3])
    with pytest.raises(ValueError, match="utterance is"):
        m.align_batch([(x, x_lens)], 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.align_batch([u, u], [3, 4])


def test_rank_by_is_checked_before_any_engine():
    from valle_amd.models import VALLE

    m = VALLE(128, 2, 2, logprobs=True, max_batch=2).eval()
    x, x_lens, y = torch.randint(3, 50, (1, 6)), torch.tensor([6]), torch.randint(0, 1024, (1, 10, 8))
    with pytest.raises(ValueError, match="rank_by"):
        m.inference_best_of(x, x_lens, y, None, 2, rank_by="mass")
