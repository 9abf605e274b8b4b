"""-m gpu: the fused PSNR / SSIM metric (csrc/ssim.hip: savfi_psnr_ssim_f32) and the frame writer (csrc/frames.hip:
savfi_frames_f32_to_u8) through the C ABI and through hip_ops, against the float64 restatement of tests/metrics_ref.py.

Gates (the rule of tests/test_ssim_gpu.py).
  sq_sum  equals the restatement's integer S exactly.
  mse     within one fp32 ulp of S / (65025 n).
  SSIM    |kernel - float64| <= max(3 E_kind, 2.4e-7): E_kind = the largest |reference fp32 - float64| of the content kind over all
          sizes and seeds 0..2 (tools/gen_golden_metrics.py, tests/golden/metrics.npz); 3 is the factor the suite grants over reference
          spread (K_SPREAD in tests/test_fullsize_gpu.py); the floor is 4 ulp of a value of order 1.

MEASURED (MI355X; worst SSIM error per kind over every METRIC_PARITY line of this file, against the gate; the run is in
profiles/metrics_parity.txt):
  kind     SSIM error   gate
  noise    1.478e-07    2.374e-06   (11 x 11, C = 3)
  smooth   1.546e-06    1.292e-05   (11 x 11, C = 1)
  near     1.405e-06    1.152e-05   (11 x 11, C = 1)
  wide     4.264e-07    4.119e-06   (12 x 75, C = 3)
  ties     1.903e-07    4.952e-06   (11 x 11, C = 1)
The kernel uses an eighth to a twenty-fifth of the gate; the errors are worst at the smallest images (one SSIM position per channel,
where the cancellation in E[x^2] - mu^2 of values up to 255^2 is not averaged) and below 1e-7 at the full sizes.  S was exact and the
mse at most 0.50 ulp off in every case; identical pairs gave S = 0 and SSIM = 1.0 exactly.
"""
import numpy as np
import pytest
import torch

from meta_interpolation_amd import _hip, hip_ops, utils
from tests import metrics_ref as M
from tests.helpers import golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = golden("metrics")
FLOOR, K = 4 * 2.0 ** -24, 3.0


def gate(kind):
    return max(K * float(GOLD['E_' + kind]), FLOOR)


def offset_copy(t, off, dtype=torch.float32):
    """A contiguous device copy of `t` whose first element sits `off` elements past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 16, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size() * off and view.is_contiguous()
    return view


def run_abi(pred, tgt, off=(0, 0), want_sq=True):
    """The entry point on raw pointers, into poisoned buffers.  -> (mse cpu [rows], ssim cpu [rows], S list of int)"""
    lib, st = _hip.lib(), _hip.current_stream()
    rows, C, H, W = pred.shape
    p, t = offset_copy(pred, off[0]), offset_copy(tgt, off[1])
    res = torch.full((rows, 2), float('nan'), device=DEV)
    sq = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    scratch = torch.full((int(lib.savfi_psnr_ssim_scratch_bytes(rows, C, H, W)),), 0xff, dtype=torch.uint8, device=DEV)
    _hip.check(lib.savfi_psnr_ssim_f32(p.data_ptr(), t.data_ptr(), res.data_ptr(), sq.data_ptr() if want_sq else None, scratch.data_ptr(),
                                       rows, C, H, W, st), "savfi_psnr_ssim_f32")
    torch.cuda.synchronize()
    res = res.cpu()
    return res[:, 0].clone(), res[:, 1].clone(), sq.cpu().tolist()


def check(kind, what, got, S64, mse64, ssim64):
    """Print the figures, then hold them to the gates."""
    mse, ssim, S = got
    e = float(np.abs(ssim.double().numpy() - ssim64).max())
    ulps = float(np.max(np.abs(mse.double().numpy() - mse64) / np.spacing(np.maximum(mse64, 2.0 ** -126).astype(np.float32)).astype(np.float64)))
    print('METRIC_PARITY kind=%s case=%s e_ssim=%.3e gate=%.3e mse_ulps=%.2f S_exact=%s' % (kind, what, e, gate(kind), ulps, S == S64))
    assert S == S64, (what, S, S64)
    assert ulps <= 1.0, (what, ulps)
    assert e <= gate(kind), (what, e, gate(kind))


@pytest.mark.parametrize("size", M.TILE_SIZES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize("kind", M.KINDS)
def test_tile_boundary_sizes_match_float64(kind, size):
    H, W = size
    for C in (1, 3):
        pred, tgt, S64, mse64, ssim64 = M.case(kind, 1, C, H, W, 0)
        name = M.case_name(kind, C, H, W, 0)
        assert S64[0] == int(GOLD[name + '/S'])                     # the inputs are the ones the reference saw
        got = run_abi(pred, tgt)
        check(kind, name, got, S64, mse64, ssim64)
        # and the reference's own fp32 values are as far away as its error plus ours allows
        assert abs(float(got[1]) - float(GOLD[name + '/ssim'])) <= gate(kind) + float(GOLD[name + '/e_ref'])
        assert abs(M.psnr(float(got[0])) - float(GOLD[name + '/psnr'])) <= 1e-3           # CONTRACT['psnr'] of tests/test_fullsize_gpu.py


@pytest.mark.parametrize("kind,size", [('wide', (256, 448)), ('near', (720, 1280))], ids=lambda v: v if isinstance(v, str) else '%dx%d' % v)
def test_full_sizes_match_float64(kind, size):
    H, W = size
    pred, tgt, S64, mse64, ssim64 = M.case(kind, 1, 3, H, W, 0)
    name = M.case_name(kind, 3, H, W, 0)
    got = run_abi(pred, tgt)
    check(kind, name, got, S64, mse64, ssim64)
    assert abs(float(got[1]) - float(GOLD[name + '/ssim'])) <= gate(kind) + float(GOLD[name + '/e_ref'])


@pytest.mark.parametrize("rows,size", [(4, (27, 75)), (8, (37, 53)), (4, (64, 96)), (8, (12, 140))])
@pytest.mark.parametrize("kind", ['near', 'ties'])
def test_rows_are_independent_and_a_nan_poisons_its_row_only(kind, rows, size):
    H, W = size
    pred, tgt, S64, mse64, ssim64 = M.case(kind, rows, 3, H, W, 1)
    assert len(set(S64)) == rows                                     # every row different
    got = run_abi(pred, tgt)
    check(kind, 'rows n%d %dx%d' % (rows, H, W), got, S64, mse64, ssim64)
    for r, where in ((1, (0, 0, 0)), (rows - 1, (2, H - 1, W - 1)), (2, (1, H // 2, W - 11))):
        for side in (0, 1):                                           # in the prediction, in the target
            pair = [pred.clone(), tgt.clone()]
            pair[side][(r,) + where] = float('nan')
            mse, ssim, S = run_abi(*pair)
            keep = [i for i in range(rows) if i != r]
            assert torch.isnan(mse[r]) and torch.isnan(ssim[r]) and S[r] == -1
            assert torch.equal(mse[keep], got[0][keep]) and torch.equal(ssim[keep], got[1][keep]) and [S[i] for i in keep] == [S64[i] for i in keep]


@pytest.mark.parametrize("off", [(1, 0), (2, 3), (3, 1), (0, 2)])
@pytest.mark.parametrize("size", [(37, 53), (64, 64), (40, 76)], ids=lambda s: '%dx%d' % s)
def test_operands_off_16_byte_alignment(off, size):
    H, W = size
    pred, tgt, S64, mse64, ssim64 = M.case('wide', 2, 3, H, W, 2)
    a = run_abi(pred, tgt)
    b = run_abi(pred, tgt, off=off)
    # the scalar loads bring the same values and every sum keeps its association: identical bits
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    check('wide', 'offset %s %dx%d' % (off, H, W), b, S64, mse64, ssim64)


def test_results_are_bit_reproducible_and_survive_graph_capture():
    pred, tgt, S64, mse64, ssim64 = M.case('near', 4, 3, 64, 96, 0)
    a, b = run_abi(pred, tgt), run_abi(pred, tgt)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    no_sq = run_abi(pred, tgt, want_sq=False)                         # sq_sum is optional
    assert torch.equal(a[0], no_sq[0]) and torch.equal(a[1], no_sq[1]) and no_sq[2] == [-7] * 4
    static_p, static_t = pred.to(DEV), tgt.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip_ops.psnr_ssim(static_p, static_t, want_sq_sum=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mse_g, ssim_g, sq_g = hip_ops.psnr_ssim(static_p, static_t, want_sq_sum=True)
    for it, (kind, seed) in enumerate((('near', 0), ('ties', 3), ('same', 1))):          # replays on changed inputs: no host decision
        p2, t2, S2, mse2, ssim2 = M.case(kind, 4, 3, 64, 96, seed)
        static_p.copy_(p2.to(DEV))
        static_t.copy_(t2.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        mse_e, ssim_e, sq_e = hip_ops.psnr_ssim(static_p.clone(), static_t.clone(), want_sq_sum=True)
        assert torch.equal(mse_g, mse_e) and torch.equal(ssim_g, ssim_e) and torch.equal(sq_g, sq_e), it
        assert sq_g.cpu().tolist() == S2
        if it == 0:
            assert torch.equal(mse_g.cpu(), a[0]) and torch.equal(ssim_g.cpu(), a[1])
        if kind == 'same':
            assert ssim_g.cpu().tolist() == [1.0] * 4 and mse_g.cpu().tolist() == [0.0] * 4


@pytest.mark.parametrize("rows,C,size", [(1, 3, (11, 11)), (1, 1, (37, 53)), (1, 3, (64, 64)), (4, 3, (27, 75)), (1, 3, (256, 448)),
                                         (1, 3, (720, 1280))])
def test_identical_pair_gives_zero_error_and_ssim_one(rows, C, size):
    H, W = size
    pred, tgt = M.make_pair('same', rows, C, H, W, 0)
    mse, ssim, S = run_abi(pred, tgt)
    print('METRIC_IDENTICAL %dx%dx%dx%d S=%s ssim=%s' % (rows, C, H, W, S, ssim.tolist()))
    assert S == [0] * rows and mse.tolist() == [0.0] * rows and ssim.tolist() == [1.0] * rows
    # values that differ before quantisation and not after it are identical too
    t2 = M.quantize(tgt) / 255.0
    mse, ssim, S = run_abi(pred, t2)
    assert S == [int(((M.quantize(pred[r]).double() - M.quantize(t2[r]).double()) ** 2).sum()) for r in range(rows)]
    if S == [0] * rows:
        assert ssim.tolist() == [1.0] * rows


def test_argument_errors():
    lib, st = _hip.lib(), _hip.current_stream()
    t = torch.zeros(3 * 16 * 16, device=DEV)
    p = t.data_ptr()
    assert lib.savfi_psnr_ssim_f32(p, p, p, p, p, 1, 3, 10, 16, st) == -2          # SAVFI_E_SHAPE
    assert lib.savfi_psnr_ssim_f32(p, p, p, p, p, 1, 3, 16, 10, st) == -2
    assert lib.savfi_psnr_ssim_f32(p, p, p, p, p, 0, 3, 16, 16, st) == -2
    assert lib.savfi_psnr_ssim_scratch_bytes(1, 3, 10, 16) == -2
    assert lib.savfi_psnr_ssim_f32(None, p, p, p, p, 1, 3, 16, 16, st) == -1       # SAVFI_E_NULL
    assert lib.savfi_psnr_ssim_f32(p, None, p, p, p, 1, 3, 16, 16, st) == -1
    assert lib.savfi_psnr_ssim_f32(p, p, None, p, p, 1, 3, 16, 16, st) == -1
    assert lib.savfi_psnr_ssim_f32(p, p, p, p, None, 1, 3, 16, 16, st) == -1
    assert lib.savfi_psnr_ssim_f32(p, p, p, p, p, 30000, 3, 16, 16, st) == -4      # SAVFI_E_TOOBIG
    assert lib.savfi_psnr_ssim_scratch_bytes(30000, 3, 16, 16) == -4
    u = torch.zeros(64, dtype=torch.uint8, device=DEV).data_ptr()
    assert lib.savfi_frames_f32_to_u8(None, u, 1, 3, 4, 4, st) == -1
    assert lib.savfi_frames_f32_to_u8(p, None, 1, 3, 4, 4, st) == -1
    assert lib.savfi_frames_f32_to_u8(p, u, 0, 3, 4, 4, st) == -2
    assert lib.savfi_frames_f32_to_u8(p, u, 1, 3, 0, 4, st) == -2
    assert lib.savfi_frames_f32_to_u8(p, u, 1, 2, 4, 4, st) == -3                  # SAVFI_E_UNSUPPORTED
    torch.cuda.synchronize()


def test_hip_ops_surface_and_the_path_selection():
    pred, tgt, S64, mse64, ssim64 = M.case('near', 3, 3, 48, 64, 0)
    mse, ssim, sq = hip_ops.psnr_ssim(pred.to(DEV).requires_grad_(), tgt.to(DEV), want_sq_sum=True)
    assert mse.shape == (3,) and ssim.shape == (3,) and not mse.requires_grad and mse[0].dim() == 0
    check('near', 'hip_ops.psnr_ssim', (mse.cpu(), ssim.cpu(), sq.cpu().tolist()), S64, mse64, ssim64)
    # views that are not contiguous are made so
    wide_p, wide_t = torch.zeros(3, 3, 48, 80, device=DEV), torch.zeros(3, 3, 48, 80, device=DEV)
    wide_p[..., 5:69], wide_t[..., 5:69] = pred.to(DEV), tgt.to(DEV)
    mse2, ssim2 = hip_ops.psnr_ssim(wide_p[..., 5:69], wide_t[..., 5:69])
    assert torch.equal(mse2, mse) and torch.equal(ssim2, ssim)
    # utils.psnr_ssim_rows takes the kernel for device tensors and utils' own composition for host tensors; both within the contract
    mse3, ssim3 = utils.psnr_ssim_rows(pred.to(DEV), tgt.to(DEV))
    assert torch.equal(mse3, mse) and torch.equal(ssim3, ssim)
    mse_c, ssim_c = utils.psnr_ssim_rows(pred, tgt)
    for r in range(3):
        assert abs(M.psnr(float(mse[r])) - M.psnr(float(mse_c[r]))) <= 1e-3 and abs(float(ssim[r]) - float(ssim_c[r])) <= 1e-4
    with pytest.raises(ValueError):
        hip_ops.psnr_ssim(pred.to(DEV)[:, :, :10], tgt.to(DEV)[:, :, :10])
    with pytest.raises(TypeError):
        hip_ops.psnr_ssim(pred.to(DEV).double(), tgt.to(DEV).double())
    # below the window: the composition, on the device
    mse4, ssim4 = utils.psnr_ssim_rows(pred.to(DEV)[:, :, :9], tgt.to(DEV)[:, :, :9])
    assert abs(float(ssim4[0]) - float(utils.psnr_ssim_rows(pred[:, :, :9], tgt[:, :, :9])[1][0])) <= 1e-4


# ------------------------------------------------------------------------------------------------------------------------
# the frame writer
# ------------------------------------------------------------------------------------------------------------------------
def expected_bytes(x):
    """[N,C,H,W] fp32 on the host -> uint8 [N,H,W,C]: utils.save_image's own arithmetic."""
    q = utils.quantize(x.mul(255))
    assert not torch.isnan(q).any()
    return q.to(torch.uint8).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("size", [(11, 11), (12, 75), (37, 53), (64, 64), (26, 140)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize("kind", M.KINDS + ('same',))
def test_writer_bytes_equal_torch_quantize_exactly(kind, size):
    H, W = size
    lib, st = _hip.lib(), _hip.current_stream()
    for C in (1, 3):
        pred, tgt = M.make_pair(kind, 2, C, H, W, 0)
        for x in (pred, tgt):
            want = expected_bytes(x)
            assert torch.equal(hip_ops.frames_to_u8(x.to(DEV)).cpu(), want)
            for off_src, off_dst in ((1, 0), (2, 1), (3, 3), (0, 2)):          # misaligned source, misaligned destination
                src = offset_copy(x, off_src)
                dst = offset_copy(torch.full(want.shape, 0x5a, dtype=torch.uint8), off_dst, torch.uint8)
                _hip.check(lib.savfi_frames_f32_to_u8(src.data_ptr(), dst.data_ptr(), 2, C, H, W, st), "savfi_frames_f32_to_u8")
                torch.cuda.synchronize()
                assert torch.equal(dst.cpu(), want), (kind, C, H, W, off_src, off_dst)


def test_writer_shapes_and_save_image(tmp_path):
    from PIL import Image
    pred, _ = M.make_pair('wide', 1, 3, 37, 53, 1)
    x = pred[0].to(DEV)
    assert torch.equal(hip_ops.frames_to_u8(x).cpu(), expected_bytes(pred)[0])                                   # [C,H,W] -> [H,W,C]
    assert torch.equal(hip_ops.frames_to_u8(x[1]).cpu(), expected_bytes(pred[:, 1:2])[0, :, :, 0])               # [H,W] -> [H,W]
    assert torch.equal(hip_ops.frames_to_u8(x[:, :, 3:40]).cpu(), expected_bytes(pred[:, :, :, 3:40])[0])        # a view
    nan = pred.clone()
    nan[0, 1, 5, 7] = float('nan')
    got = hip_ops.frames_to_u8(nan.to(DEV)).cpu()
    assert int(got[0, 5, 7, 1]) == 0
    got[0, 5, 7, 1] = expected_bytes(pred)[0, 5, 7, 1]
    assert torch.equal(got, expected_bytes(pred))
    with pytest.raises(ValueError):
        hip_ops.frames_to_u8(torch.zeros(1, 2, 8, 8, device=DEV))
    # utils.save_image: the file written from the device tensor holds the bytes of the one written from the host tensor
    utils.save_image(x, str(tmp_path / 'dev.png'))
    utils.save_image(pred[0], str(tmp_path / 'host.png'))
    utils.save_image(x[0], str(tmp_path / 'dev_l.png'))
    utils.save_image(pred[0, 0], str(tmp_path / 'host_l.png'))
    for a, b in (('dev.png', 'host.png'), ('dev_l.png', 'host_l.png')):
        assert np.array_equal(np.asarray(Image.open(str(tmp_path / a))), np.asarray(Image.open(str(tmp_path / b))))
