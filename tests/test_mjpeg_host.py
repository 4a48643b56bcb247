"""Motion-JPEG timelapse video, the parts that need no GPU: the tables, the fixed-point DCT against a float64 one, the twin
encoder of tests/jpeg_ref.py against PIL's decoder and PIL's own encoder, byte stuffing, the AVI container, the refusals, the
CLI / TOML surface, the wiring in ``main.style_transfer`` and in the runner, and the argument checks of the four entry points."""
from __future__ import annotations

import io
import logging
import os
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.fft
import torch
from PIL import Image

from style_transfer_visualizer_amd import _lib, cli, core_model, gif, image_io, mjpeg, optimization, runtime
from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd import main as stv_main
from style_transfer_visualizer_amd.optimization import OptimizationCallbacks, OptimizationRunner
from style_transfer_visualizer_amd.type_defs import InputPaths
from tests import jpeg_ref as jr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 96, 80


def _noise() -> np.ndarray:
    return np.random.default_rng(7).integers(64, 128, size=(H, W, 3)).astype(np.uint8)


def _gradient() -> np.ndarray:
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([x * 255 // (W - 1), y * 255 // (H - 1), (x + y) * 255 // (H + W - 2)], axis=2).astype(np.uint8)


def _smooth() -> np.ndarray:
    """An image-like frame: a few low-frequency waves per channel, an edge, and a little grain."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    rng = np.random.default_rng(5)
    r = 128 + 80 * np.sin(x / 11.0) * np.cos(y / 17.0)
    g = 110 + 60 * np.cos((x + y) / 23.0) + 40 * (x > 50)
    b = 90 + 70 * np.sin(y / 9.0 + x / 31.0)
    out = np.stack([r, g, b], axis=2) + rng.normal(0, 3, size=(H, W, 3))
    return np.clip(np.round(out), 0, 255).astype(np.uint8)


FRAMES = {"noise": _noise, "gradient": _gradient, "smooth": _smooth}


# ---- tables ----------------------------------------------------------------------------------------------------------------

def test_quality_map_and_tables_equal_pil():
    assert [mjpeg.jpeg_quality(q) for q in range(1, 11)] == [min(95, 10 * q + 5) for q in range(1, 11)]
    with pytest.raises(ValueError, match="between 1 and 10"):
        mjpeg.jpeg_quality(11)
    img = Image.fromarray(_gradient())
    for q in range(1, 11):
        Q = mjpeg.jpeg_quality(q)
        buf = io.BytesIO()
        img.save(buf, "JPEG", quality=Q, subsampling=2, optimize=False)
        with Image.open(io.BytesIO(buf.getvalue())) as im:
            theirs = {k: list(v) for k, v in im.quantization.items()}
        mine = mjpeg.quant_tables(Q)
        assert mine.shape == (2, 64) and mine.min() >= 1 and mine.max() <= 255
        # PIL reports the tables row-major (it undoes the file's zigzag order) since Pillow 8.3; a file holds them zigzag
        natural = [theirs[k] == mine[k].tolist() for k in (0, 1)]
        zigzag = [theirs[k] == mine[k][list(mjpeg.ZIGZAG)].tolist() for k in (0, 1)]
        assert natural == [True, True] or zigzag == [True, True], f"quality {Q}"
    assert mjpeg.quant_tables(50)[0].tolist() == list(mjpeg.LUMA_BASE)
    assert mjpeg.quant_tables(1).max() == 255 and mjpeg.quant_tables(100).max() == 1          # both clamps


def test_the_huffman_tables_are_the_ones_pil_writes():
    buf = io.BytesIO()
    Image.fromarray(_gradient()).save(buf, "JPEG", quality=75, subsampling=2, optimize=False)
    theirs = _segments(buf.getvalue())["dht"]
    for cls, tid, (bits, vals) in mjpeg.HUFFMAN_TABLES:
        assert theirs[cls << 4 | tid] == (tuple(bits), tuple(vals))
        assert sum(bits) == len(vals)


def test_the_kernel_source_holds_the_same_tables():
    text = open(os.path.join(ROOT, "style_transfer_visualizer_amd", "csrc", "jpeg.hip")).read()

    def array(name: str) -> tuple[int, ...]:
        body = re.search(name + r"\[\d+\] = \{(.*?)\};", text, flags=re.S).group(1)
        return tuple(int(v, 0) for v in body.replace("\n", " ").split(",") if v.strip())
    for prefix, table in (("kDcLum", mjpeg.DC_LUMA), ("kDcChr", mjpeg.DC_CHROMA), ("kAcLum", mjpeg.AC_LUMA), ("kAcChr", mjpeg.AC_CHROMA)):
        assert array(prefix + "Bits") == tuple(table[0])
        assert array(prefix[:3] + "Vals" if prefix.startswith("kDc") else prefix + "Vals") == tuple(table[1])


def test_the_dct_table_equals_its_float64_construction():
    u, x = np.mgrid[0:8, 0:8].astype(np.float64)
    c = np.where(u == 0, 1 / np.sqrt(2.0), 1.0)
    want = np.rint(8192 * c / 2 * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int64)
    assert np.array_equal(np.array(_lib.JPEG_DCT_TABLE), want)
    assert want[0].tolist() == [2896] * 8 and want[1, :4].tolist() == [4017, 3406, 2276, 799]
    header = open(os.path.join(ROOT, "include", "stv.h")).read()
    body = header[header.index("#define STV_JPEG_DCT_TABLE"):header.index("/* launch constants: stv_jpeg_dct")]
    assert [int(v) for v in re.findall(r"-?\d+", body.replace("STV_JPEG_DCT_TABLE", ""))] == want.reshape(-1).tolist()
    zz = np.array(mjpeg.ZIGZAG)
    assert sorted(zz.tolist()) == list(range(64)) and zz[:10].tolist() == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24] and zz[-3:].tolist() == [55, 62, 63]


# ---- the fixed-point DCT ---------------------------------------------------------------------------------------------------

def _extreme_blocks() -> np.ndarray:
    """For every coefficient (v, u) the two blocks of -128 / 127 that follow the sign of its basis function, and its negative:
    128 blocks, the largest magnitude each coefficient can take."""
    T = jr.T
    out = []
    for v in range(8):
        for u in range(8):
            sign = np.sign(np.outer(T[v], T[u]))
            out += [np.where(sign > 0, 127, -128), np.where(sign > 0, -128, 127)]
    return np.array(out, dtype=np.int64)


def _dct_inputs() -> np.ndarray:
    rng = np.random.default_rng(3)
    return np.concatenate([rng.integers(-128, 128, size=(4000, 8, 8)), rng.integers(0, 2, size=(4000, 8, 8)) * 255 - 128, _extreme_blocks()])


DCT_MEASURED_ERROR = 0.24       # the largest |b / 2^18 - dctn| seen over _dct_inputs(); asserted with a margin of 0.05


def test_the_fixed_point_dct_against_float64():
    s = _dct_inputs()
    a, a1, b = jr.dct_stages(s)
    assert int(np.abs(a).max()) <= 2965504 and int(np.abs(a1).max()) <= 11584 and int(np.abs(b).max()) <= 268378112      # int32
    assert int(np.abs(b).max()) + (255 << 17) < 2 ** 31                                                                  # the rounding add
    ref = scipy.fft.dctn(s.astype(np.float64), axes=(1, 2), norm="ortho")           # ref[n, v, u]
    err = float(np.abs(b / 2.0 ** 18 - ref).max())
    print(f"fixed-point DCT: max |error| = {err:.4f}")
    assert err <= DCT_MEASURED_ERROR + 0.05
    for q in range(1, 11):
        tabs = mjpeg.quant_tables(mjpeg.jpeg_quality(q)).reshape(2, 8, 8)
        for tab in tabs:
            got = jr.quantise(b, tab)
            exact = np.abs(ref) / tab
            want = np.sign(ref) * np.floor(exact + 0.5)
            want = np.clip(want, -1023, 1023)
            want[:, 0, 0] = np.clip((np.sign(ref) * np.floor(exact + 0.5))[:, 0, 0], -1024, 1023)
            diff = np.abs(got - want)
            frac = float((diff != 0).mean())
            print(f"q = {q}: {100 * frac:.3f} % of the coefficients differ from the float64 rounding")
            assert diff.max() <= 1
            assert frac < (0.025 if q == 1 else 0.01)


def test_the_twin_covers_edges_and_block_order():
    """17x15 pixels: two MCUs, one above the other.  The last row (16) is white and fills the second MCU; the last column
    (14) of the first MCU is red and is replicated into column 15."""
    frame = np.zeros((17, 15, 3), dtype=np.uint8)
    frame[:16, 14] = (255, 0, 0)
    frame[16] = 255
    s = jr.samples(frame)
    assert s.shape == (12, 8, 8)
    assert (s[6:10] == 127).all() and (s[10:12] == 0).all()     # the white MCU: Y = 255, Cb = Cr = 128
    assert (s[0] == -128).all() and (s[2] == -128).all()        # Y00, Y10 of the first MCU: black
    for k in (1, 3):                                            # Y01, Y11: columns 14 and 15 carry red's luminance, 76
        assert (s[k][:, :6] == -128).all() and (s[k][:, 6:] == 76 - 128).all()
    assert (s[4][:, :7] == 0).all() and (s[4][:, 7] == 85 - 128).all()         # Cb: the 2x2 group of columns 14, 15 is red
    assert (s[5][:, :7] == 0).all() and (s[5][:, 7] == 255 - 128).all()        # Cr of red is 255
    coefs = jr.dct_quant(frame, mjpeg.quant_tables(50))
    assert coefs.shape == (12, 64) and coefs.dtype == np.int16
    # flat blocks: a DC term alone.  127 * 8 / 16 = 63.5 is a tie in exact arithmetic; the fixed-point DC is 1015.8 (T[0] is
    # 2896 for 2896.31), so this is one of the coefficients that round the other way
    assert coefs[6, 0] == 63 and coefs[0, 0] == -64 and not coefs[6:, 1:].any()
    assert coefs[1, 1] != 0 and coefs[1, 2] == 0               # a step along x: zigzag 1 is (v, u) = (0, 1), zigzag 2 is (1, 0)


# ---- the twin's files against PIL ------------------------------------------------------------------------------------------

def _segments(data: bytes) -> dict:
    """Marker order, the DQT and DHT payloads and the SOF0 fields of a JPEG file, up to SOS."""
    assert data[:2] == b"\xff\xd8"
    out = {"order": ["SOI"], "dqt": {}, "dht": {}}
    names = {0xE0: "APP0", 0xDB: "DQT", 0xC0: "SOF0", 0xC4: "DHT", 0xDA: "SOS"}
    at = 2
    while True:
        assert data[at] == 0xFF
        marker, size = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        body = data[at + 4:at + 2 + size]
        out["order"].append(names.get(marker, hex(marker)))
        if marker == 0xDB:
            while body:
                out["dqt"][body[0]] = list(body[1:65])
                body = body[65:]
        elif marker == 0xC4:
            while body:
                bits = tuple(body[1:17])
                out["dht"][body[0]] = (bits, tuple(body[17:17 + sum(bits)]))
                body = body[17 + sum(bits):]
        elif marker == 0xC0:
            out["sof"] = (body[0], int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big"), body[5], list(body[6:15]))
        elif marker == 0xE0:
            out["app0"] = body
        elif marker == 0xDA:
            out["sos"] = body
            out["scan_at"] = at + 2 + size
            return out
        at += 2 + size


def _psnr(a: np.ndarray, b: np.ndarray) -> float:
    return float(10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


@pytest.mark.parametrize("name", list(FRAMES))
def test_pil_opens_the_twins_files(name):
    frame = FRAMES[name]()
    qtabs = mjpeg.quant_tables(75)
    data = jr.encode_frame(frame, qtabs)
    seg = _segments(data)
    assert seg["order"] == ["SOI", "APP0", "DQT", "DQT", "SOF0", "DHT", "DHT", "DHT", "DHT", "SOS"] and data[-2:] == b"\xff\xd9"
    assert seg["app0"][:7] == b"JFIF\x00\x01\x01"
    assert seg["sof"] == (8, H, W, 3, [1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert seg["dqt"] == {t: qtabs[t][list(mjpeg.ZIGZAG)].tolist() for t in (0, 1)}
    assert set(seg["dht"]) == {0x00, 0x10, 0x01, 0x11}
    with Image.open(io.BytesIO(data)) as im:
        im.load()
        assert im.size == (W, H) and im.mode == "RGB" and im.format == "JPEG"
        theirs = {k: list(v) for k, v in im.quantization.items()}
        assert theirs in ({t: qtabs[t].tolist() for t in (0, 1)}, seg["dqt"])


@pytest.mark.parametrize("Q", [15, 55, 95])
@pytest.mark.parametrize("name", list(FRAMES))
def test_psnr_and_size_against_pils_encoder(name, Q):
    """The mistakes this code can make - table orientation, zigzag, level shift, chroma siting - cost several dB; encoder
    rounding costs hundredths: the twin may be at most 0.5 dB below PIL.  Same quantisation and Huffman tables, so only the
    coefficients that round differently move the size: at most 1.05 of PIL's."""
    frame = FRAMES[name]()
    mine = jr.encode_frame(frame, mjpeg.quant_tables(Q))
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "JPEG", quality=Q, subsampling=2, optimize=False)
    theirs = buf.getvalue()
    with Image.open(io.BytesIO(mine)) as a, Image.open(io.BytesIO(theirs)) as b:
        mine_db, pil_db = _psnr(np.array(a.convert("RGB")), frame), _psnr(np.array(b.convert("RGB")), frame)
    print(f"{name} Q={Q}: PSNR {mine_db:.3f} dB (PIL {pil_db:.3f} dB), {len(mine)} bytes (PIL {len(theirs)})")
    assert mine_db >= pil_db - 0.5
    assert len(mine) <= 1.05 * len(theirs)


def test_stuff():
    assert mjpeg.stuff(b"") == b"" and mjpeg.stuff(b"\x00\x01\xfe") == b"\x00\x01\xfe"
    assert mjpeg.stuff(b"\xff\x12\x34") == b"\xff\x00\x12\x34"                # at the start
    assert mjpeg.stuff(b"\x12\x34\xff") == b"\x12\x34\xff\x00"                # at the end
    assert mjpeg.stuff(b"\x12\xff\xff\x34") == b"\x12\xff\x00\xff\x00\x34"    # doubled
    assert mjpeg.stuff(b"\xff\x00") == b"\xff\x00\x00"                        # a zero that was data stays
    assert mjpeg.stuff(bytearray(b"\xff")) == b"\xff\x00" and mjpeg.stuff(np.array([255, 1], dtype=np.uint8).tobytes()) == b"\xff\x00\x01"


# ---- the container ---------------------------------------------------------------------------------------------------------

def _jpegs(n: int) -> list[bytes]:
    qtabs = mjpeg.quant_tables(55)
    return [jr.encode_frame(np.roll(_smooth(), 7 * i, axis=1), qtabs) for i in range(n)]


def test_write_avi_round_trip(tmp_path):
    frames = _jpegs(3)
    frames[1] += b"\x00" if len(frames[1]) % 2 == 0 else b""        # at least one odd length: a padded chunk
    assert any(len(f) % 2 for f in frames)
    info = mjpeg.video_info("A title", None)
    assert info["artist"] == "Style Transfer Visualizer" and info["software"].startswith("style_transfer_visualizer_amd v")
    path = tmp_path / "sub" / "t.avi"
    assert mjpeg.write_avi(path, frames, W, H, 12, info) == 3
    data = path.read_bytes()
    avi = jr.read_avi(data)
    usec, _, _, flags, total, _, streams, suggested, width, height = avi["avih"][:10]
    assert (usec, flags & 0x10, total, streams, width, height) == (1000000 // 12, 0x10, 3, 1, W, H) and suggested == max(map(len, frames))
    fourccs, strh = avi["strh"]
    assert fourccs == b"vidsMJPG"
    assert (strh[4], strh[5], strh[7], strh[8]) == (1, 12, 3, max(map(len, frames)))        # scale, rate, length, buffer size
    assert strh[-2:] == (W, H)
    size, bw, bh, planes, bitcount, compression, image_bytes = avi["strf"][:7]
    assert (size, bw, bh, planes, bitcount, compression, image_bytes) == (40, W, H, 1, 24, b"MJPG", W * H * 3)
    assert avi["info"] == {b"INAM": "A title", b"IART": "Style Transfer Visualizer", b"ISFT": info["software"]}
    assert [c["id"] for c in avi["frames"]] == [b"00dc"] * 3
    assert [c["data"] for c in avi["frames"]] == frames
    assert all(c["at"] % 2 == 0 for c in avi["frames"])                                     # even padding keeps every chunk aligned
    assert len(avi["index"]) == 3
    for (ckid, flags, offset, length), chunk in zip(avi["index"], avi["frames"], strict=True):
        assert ckid == b"00dc" and flags == 0x10 and length == chunk["size"]
        at = avi["movi_at"] + offset                                                        # from the "movi" tag
        assert at == chunk["at"] and data[at:at + 4] == b"00dc"
    for chunk in avi["frames"]:
        with Image.open(io.BytesIO(chunk["data"])) as im:
            im.load()
            assert im.size == (W, H)


def test_the_size_cap_closes_the_file_at_the_last_frame_that_fits(tmp_path, monkeypatch, caplog):
    frames = _jpegs(4)
    path = tmp_path / "full.avi"
    mjpeg.write_avi(path, frames[:2], W, H, 10, {})
    two = path.stat().st_size
    monkeypatch.setattr(mjpeg, "AVI_MAX_BYTES", two + 100)          # the third frame does not fit
    with caplog.at_level(logging.WARNING, logger="style_transfer"):
        assert mjpeg.write_avi(path, frames, W, H, 10, {}) == 2
    (message,) = caplog.messages
    assert "2 of 4 frames" in message
    assert path.stat().st_size == two <= mjpeg.AVI_MAX_BYTES
    avi = jr.read_avi(path.read_bytes())
    assert avi["avih"][4] == 2 and len(avi["frames"]) == 2 and len(avi["index"]) == 2
    monkeypatch.undo()
    assert mjpeg.AVI_MAX_BYTES == 2 ** 31 - 2 ** 20


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_refusals_name_their_values():
    assert mjpeg.store_bytes(10, 17, 15) == 10 * 32 * 16 * 3 and mjpeg.store_bytes(1, 512, 512) == 3 * 512 * 512
    with pytest.raises(ValueError, match=r"70000x100"):
        mjpeg.check_frame_size(100, 70000)
    with pytest.raises(ValueError, match=r"100x65536"):
        mjpeg.check_frame_size(65536, 100)
    with pytest.raises(ValueError, match="100 frames of 4096x4096 pixels need 5033164800 bytes.*larger --save-every"):
        mjpeg.check_budget(100, 4096, 4096)
    gif_text, mjpeg_text = [], []
    for module, sink in ((gif, gif_text), (mjpeg, mjpeg_text)):
        with pytest.raises(ValueError) as err:
            module.check_budget(1000, 4096, 4096)
        sink.append(re.sub(r"\d+", "N", str(err.value)).replace("GIF", "X").replace("MJPEG", "X"))
    assert gif_text == mjpeg_text                                   # the wording of the GIF's refusal
    with pytest.raises(ValueError, match="32-bit bit offsets"):
        mjpeg.check_frame_size(30000, 30000)
    with pytest.raises(ValueError, match="1..255"):
        mjpeg.jpeg_headers(16, 16, np.zeros((2, 64)))


# ---- CLI and TOML ----------------------------------------------------------------------------------------------------------

BASE = ["--content", "c.png", "--style", "s.png"]


def _cli_config(argv):
    args = cli.build_arg_parser().parse_args(argv)
    base = stv_config.ConfigLoader.load(args.config) if args.config else None
    return stv_config.build_config_from_cli(vars(args), base_config=base)


def test_cli_and_toml_round_trip(tmp_path, caplog):
    plain = _cli_config(BASE)
    assert plain.video.format == "mp4" and plain.video.create_video is True
    cfg = _cli_config([*BASE, "--video-format", "mjpeg", "--quality", "3", "--metadata-title", "T", "--metadata-artist", "A"])
    assert (cfg.video.format, cfg.video.quality, cfg.video.metadata_title, cfg.video.metadata_artist) == ("mjpeg", 3, "T", "A")
    toml = tmp_path / "c.toml"
    toml.write_text('[video]\nformat = "mjpeg"\n')
    assert _cli_config([*BASE, "--config", str(toml)]).video.format == "mjpeg"
    assert _cli_config([*BASE, "--config", str(toml), "--video-format", "mp4"]).video.format == "mp4"       # the CLI wins
    with pytest.raises(ValueError):
        stv_config.StyleTransferConfig.model_validate({"video": {"format": "webm"}})
    with pytest.raises(SystemExit):
        cli.build_arg_parser().parse_args([*BASE, "--video-format", "webm"])
    with pytest.raises(ValueError):
        stv_config.build_config_from_cli({"video_format": "webm"})
    paths = InputPaths("c.png", "s.png")
    with caplog.at_level(logging.INFO, logger="style_transfer"):
        cli.log_parameters(paths, cfg)
    assert "Video Format: mjpeg" in caplog.text
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="style_transfer"):
        cli.log_parameters(paths, plain)
    assert "Video Format" not in caplog.text                        # the default banner is the one it was


# ---- wiring in main.style_transfer -----------------------------------------------------------------------------------------

class _Recorder:
    def __init__(self):
        self.runner_args = None
        self.saved = None
        self.writers = []
        self.collectors = []
        self.prepare = None
        self.device = torch.device("cpu")


class _FakeSink:
    def __init__(self, into, path, fps, H, W, n_frames, **kw):
        self.args, self.kw, self.closed = (path, fps, H, W, n_frames), kw, 0
        into.append(self)

    def close(self):
        self.closed += 1


@pytest.fixture
def wired(monkeypatch):
    rec = _Recorder()
    img = torch.linspace(-0.5, 1.5, 3 * 16 * 24).reshape(1, 3, 16, 24)
    monkeypatch.setattr(runtime, "validate_input_paths", lambda *a, **k: None)
    monkeypatch.setattr(runtime, "setup_random_seed", lambda seed: None)
    monkeypatch.setattr(runtime, "setup_device", lambda name: rec.device)
    monkeypatch.setattr(runtime, "setup_output_directory", lambda p: Path("mock_output"))
    monkeypatch.setattr(runtime, "save_outputs", lambda *a, **k: setattr(rec, "saved", a))
    monkeypatch.setattr(image_io, "load_image_to_tensor", lambda *a, **k: img.clone())

    def prepare(*a, **k):
        rec.prepare = (len(a), dict(k))
        return "model", img.clone().requires_grad_(True), "optimizer"
    monkeypatch.setattr(core_model, "prepare_model_and_input", prepare)
    monkeypatch.setattr(mjpeg, "DeviceMjpegWriter", lambda *a, **k: _FakeSink(rec.writers, *a, **k))
    monkeypatch.setattr(gif, "DeviceGifCollector", lambda *a, **k: _FakeSink(rec.collectors, *a, **k))

    class FakeRunner:
        def __init__(self, *args, **kwargs):
            rec.runner_args = (args, kwargs)

        def run(self):
            return img.clone().requires_grad_(True), {"total_loss": [1.0]}, 3.14
    monkeypatch.setattr(optimization, "OptimizationRunner", FakeRunner)
    return rec


def _cfg(**video):
    cfg = stv_config.StyleTransferConfig.model_validate({})
    cfg.optimization.steps, cfg.optimization.seed = 10, 42
    for k, v in video.items():
        setattr(cfg.video, k, v)
    return cfg


WARNING = "Timelapse encoding is not part of the MI355X build; continuing without video/GIF"


def test_mp4_is_downgraded_with_the_existing_warning_and_nothing_new_is_entered(wired, caplog):
    wired.device = torch.device("cuda")
    cfg = _cfg(save_every=3)
    assert cfg.video.format == "mp4" and cfg.video.create_video is True
    with caplog.at_level(logging.WARNING, logger="style_transfer"):
        stv_main.style_transfer(InputPaths("a.png", "b.png"), cfg)
    (message,) = caplog.messages
    assert message == WARNING + " (pass --no-video to silence this, or inject a frame sink)."
    assert cfg.video.create_video is False and not wired.writers and wired.runner_args[1]["video_writer"] is None
    assert wired.saved[4].video_created is False and wired.saved[4].video_name is None
    mp4_prepare = wired.prepare
    assert mp4_prepare == (4, {"precision": cfg.hardware.precision})          # the keywords of today
    stv_main.style_transfer(InputPaths("a.png", "b.png"), _cfg(save_every=3, format="mjpeg", intro_enabled=False, final_frame_compare=False))
    assert wired.prepare == mp4_prepare and len(wired.writers) == 1


def test_mjpeg_creates_the_built_in_writer_under_the_references_name(wired, caplog):
    wired.device = torch.device("cuda")
    cfg = _cfg(format="mjpeg", save_every=3, fps=24, quality=3, intro_enabled=False, final_frame_compare=False, metadata_title="My title")
    with caplog.at_level(logging.WARNING, logger="style_transfer"):
        stv_main.style_transfer(InputPaths("dir/a.png", "b.png", extra_style_paths=("x/c.png",)), cfg, output_tag="_007", tag_png=False)
    assert not caplog.messages and cfg.video.create_video is True
    (writer,) = wired.writers
    assert writer.args == (Path("mock_output") / "timelapse_a_x_b+c_007.avi", 24, 16, 24, 3)      # 10 // 3 frames of the run's size
    assert writer.kw["quality"] == 3 and writer.kw["device"] == torch.device("cuda")
    assert writer.kw["info"]["title"] == "My title" and writer.kw["info"]["artist"] == mjpeg.DEFAULT_ARTIST
    assert wired.runner_args[1]["video_writer"] is writer and wired.runner_args[1]["gif_collector"] is None and writer.closed == 1
    opts = wired.saved[4]
    assert opts.video_created is True and opts.video_name == "timelapse_a_x_b+c_007.avi" and opts.gif_created is False


def test_gif_and_mjpeg_together_and_an_injected_writer_wins(wired, caplog):
    wired.device = torch.device("cuda")
    with caplog.at_level(logging.WARNING, logger="style_transfer"):
        stv_main.style_transfer(InputPaths("a.png", "b.png"), _cfg(format="mjpeg", create_gif=True, intro_enabled=False, final_frame_compare=False))
    assert not caplog.messages and len(wired.writers) == 1 and len(wired.collectors) == 1
    assert wired.saved[4].video_name == "timelapse_a_x_b.avi" and wired.saved[4].gif_name == "timelapse_a_x_b.gif"

    class Sink:
        closed = 0

        def append_data(self, frame):
            pass

        def close(self):
            self.closed += 1
    sink = Sink()
    stv_main.style_transfer(InputPaths("a.png", "b.png"), _cfg(format="mjpeg"), video_writer=sink)
    assert len(wired.writers) == 1 and wired.runner_args[1]["video_writer"] is sink and sink.closed == 1
    assert wired.saved[4].video_created is True and wired.saved[4].video_name is None


def test_intro_and_outro_flags_give_one_warning_that_names_the_silencing_flags(wired, caplog):
    wired.device = torch.device("cuda")
    with caplog.at_level(logging.WARNING, logger="style_transfer"):
        stv_main.style_transfer(InputPaths("a.png", "b.png"), _cfg(format="mjpeg"))
    (message,) = caplog.messages
    assert "--no-intro" in message and "--no-final-frame-compare" in message and len(wired.writers) == 1
    caplog.clear()
    cfg = _cli_config([*BASE, "--video-format", "mjpeg", "--no-intro", "--no-final-frame-compare"])
    cfg.optimization.steps = 10
    with caplog.at_level(logging.WARNING, logger="style_transfer"):
        stv_main.style_transfer(InputPaths("a.png", "b.png"), cfg)
    assert not caplog.messages and len(wired.writers) == 2


def test_cpu_final_only_no_video_and_a_pyramid_keep_the_writer_away(wired, caplog, monkeypatch):
    with caplog.at_level(logging.WARNING, logger="style_transfer"):
        cfg = _cfg(format="mjpeg")
        stv_main.style_transfer(InputPaths("a.png", "b.png"), cfg)                 # a CPU device
    assert sum(WARNING in m for m in caplog.messages) == 1 and len(caplog.messages) == 1 and cfg.video.create_video is False
    assert not wired.writers and wired.saved[4].video_created is False
    wired.device = torch.device("cuda")
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="style_transfer"):
        stv_main.style_transfer(InputPaths("a.png", "b.png"), _cfg(format="mjpeg", final_only=True))
        stv_main.style_transfer(InputPaths("a.png", "b.png"), _cfg(format="mjpeg", create_video=False))
    assert not caplog.messages and not wired.writers
    from style_transfer_visualizer_amd import pyramid
    seen = {}

    def fake_pyramid(*a, **k):
        seen.update(k)
        return torch.zeros(1, 3, 16, 24), {}, 0.0
    monkeypatch.setattr(pyramid, "run_pyramid", fake_pyramid)
    cfg = _cfg(format="mjpeg")
    cfg.optimization.pyramid_levels = 2
    with caplog.at_level(logging.WARNING, logger="style_transfer"):
        stv_main.style_transfer(InputPaths("a.png", "b.png"), cfg)
    assert sum(WARNING in m for m in caplog.messages) == 1 and cfg.video.create_video is False
    assert not wired.writers and seen["video_writer"] is None


def test_the_refusals_come_before_the_model(wired, monkeypatch):
    wired.device = torch.device("cuda")
    big = torch.empty(1, 3, 4096, 4096)                    # (never read: only its shape counts)
    monkeypatch.setattr(image_io, "load_image_to_tensor", lambda *a, **k: big)
    cfg = _cfg(format="mjpeg", save_every=1)
    cfg.optimization.steps = 100
    with pytest.raises(ValueError, match="100 frames of 4096x4096"):
        stv_main.style_transfer(InputPaths("a.png", "b.png"), cfg)
    assert wired.runner_args is None and wired.prepare is None and not wired.writers
    wide = torch.empty(1, 3, 2, 65536)
    monkeypatch.setattr(image_io, "load_image_to_tensor", lambda *a, **k: wide)
    with pytest.raises(ValueError, match="65536x2"):
        stv_main.style_transfer(InputPaths("a.png", "b.png"), _cfg(format="mjpeg"))
    assert wired.prepare is None


def test_save_outputs_names_the_video(tmp_path, caplog, monkeypatch):
    from style_transfer_visualizer_amd.type_defs import SaveOptions
    monkeypatch.setattr(image_io, "save_image", lambda *a, **k: None)
    opts = SaveOptions(content_name="a", style_name="b", video_name="t.avi", video_created=True, plot_losses=False)
    with caplog.at_level(logging.INFO, logger="style_transfer"):
        runtime.save_outputs(torch.zeros(1, 3, 4, 4), {}, tmp_path, 1.0, opts)
    assert f"Video saved to: {tmp_path / 't.avi'}" in caplog.text


# ---- the runner: a video writer with append_device gets the image, no host frame is formed -------------------------------------

class _TinyModel(torch.nn.Module):
    def forward(self, x):
        return [(x ** 2).mean()], [((x + 0.5) ** 2).mean()]


class _Bar:
    def update(self, n=1):
        return None

    def set_postfix(self, *a, **k):
        return None

    def close(self):
        return None


class _DeviceSink:
    def __init__(self):
        self.device_calls, self.host_frames = [], []

    def append_device(self, image, *, normalize):
        self.device_calls.append((tuple(image.shape), normalize))

    def append_data(self, frame):
        self.host_frames.append(frame)

    def close(self):
        return None


class _HostSink:
    def __init__(self):
        self.frames = []

    def append_data(self, frame):
        self.frames.append(frame)

    def close(self):
        return None


def _runner(*, steps=7, save_every=2, **kw):
    cfg = stv_config.StyleTransferConfig.model_validate({})
    cfg.optimization.steps, cfg.optimization.normalize = steps, False
    cfg.video.save_every, cfg.output.log_every = save_every, 2
    x = torch.full((1, 3, 8, 8), 0.25, requires_grad=True)
    return OptimizationRunner(_TinyModel(), x, cfg, optimizer=torch.optim.Adam([x]), progress_bar=_Bar(), **kw)


def test_a_device_video_writer_alone_needs_no_host_frame(monkeypatch):
    def forbidden(*a, **k):
        raise AssertionError("a host frame was formed")
    monkeypatch.setattr(image_io, "frame_uint8", forbidden)
    sink = _DeviceSink()
    _runner(video_writer=sink).run()
    assert sink.device_calls == [((1, 3, 8, 8), False)] * (7 // 2) and not sink.host_frames
    video, collector = _DeviceSink(), _DeviceSink()
    _runner(video_writer=video, gif_collector=collector).run()           # both on the device: still no host frame
    assert len(video.device_calls) == 3 and len(collector.device_calls) == 3 and not video.host_frames and not collector.host_frames


def test_a_callback_or_a_host_sink_brings_the_host_frame_back(monkeypatch):
    calls = []
    real = image_io.frame_uint8
    monkeypatch.setattr(image_io, "frame_uint8", lambda *a, **k: calls.append(1) or real(*a, **k))
    sink, seen = _DeviceSink(), []
    _runner(video_writer=sink, callbacks=OptimizationCallbacks(on_video_frame=lambda frame, step: seen.append((frame.shape, step)))).run()
    assert len(calls) == 3 and seen == [((8, 8, 3), 2), ((8, 8, 3), 4), ((8, 8, 3), 6)]
    assert len(sink.device_calls) == 3 and not sink.host_frames          # the device writer is not handed the host frame too
    video, collector = _DeviceSink(), _HostSink()
    _runner(video_writer=video, gif_collector=collector).run()
    assert len(collector.frames) == 3 and len(video.device_calls) == 3 and not video.host_frames
    plain = _HostSink()                                                  # a sink without append_device: as before
    _runner(video_writer=plain).run()
    assert len(plain.frames) == 3 and plain.frames[0].shape == (8, 8, 3)


# ---- ABI -------------------------------------------------------------------------------------------------------------------

def test_the_entry_points_refuse_bad_arguments_before_any_device_work():
    import ctypes
    lib = _lib.load()
    assert lib.stv_version() >= 116
    for name in ("stv_jpeg_dct", "stv_jpeg_block_bits", "stv_jpeg_scan", "stv_jpeg_emit"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert "jpeg.hip" in open(os.path.join(ROOT, "style_transfer_visualizer_amd", "csrc", "Makefile")).read()
    ERR, P = 1, 0x1000          # (a non-null, 16-byte aligned address: never dereferenced, the checks come first)
    good = (ctypes.c_int * 128)(*([16] * 128))

    def dct(frame=P, q=good, H=16, W=16, coef=P):
        return lib.stv_jpeg_dct(frame, q, H, W, coef, None)
    assert dct(frame=None) == ERR and dct(q=None) == ERR and dct(coef=None) == ERR
    assert dct(H=0) == ERR and dct(W=0) == ERR and dct(H=-1) == ERR
    assert dct(H=65536) == ERR and dct(W=65536) == ERR
    assert dct(coef=P + 2) == ERR
    for at in (0, 63, 64, 127):
        for bad in (0, 256, -1):
            q = (ctypes.c_int * 128)(*([16] * 128))
            q[at] = bad
            assert dct(q=q) == ERR

    def bits(coef=P, F=1, B=6, out=P):
        return lib.stv_jpeg_block_bits(coef, F, B, out, None)
    assert bits(coef=None) == ERR and bits(out=None) == ERR and bits(F=0) == ERR and bits(B=0) == ERR and bits(B=-6) == ERR
    assert bits(B=7) == ERR and bits(coef=P + 8) == ERR
    assert bits(B=(2 ** 32 // _lib.JPEG_MAX_BLOCK_BITS + 6) // 6 * 6) == ERR                # bit offsets past 32 bits
    assert bits(F=2 ** 20, B=6 * 2 ** 10) == ERR                                            # 2^31 blocks and more

    def scan(src=P, F=1, B=6, offsets=P, totals=P):
        return lib.stv_jpeg_scan(src, F, B, offsets, totals, None)
    assert scan(src=None) == ERR and scan(offsets=None) == ERR and scan(totals=None) == ERR
    assert scan(F=0) == ERR and scan(B=0) == ERR and scan(B=5) == ERR

    def emit(coef=P, offsets=P, base=P, F=1, B=6, stream=P, capacity=64):
        return lib.stv_jpeg_emit(coef, offsets, base, F, B, stream, capacity, None)
    assert emit(coef=None) == ERR and emit(offsets=None) == ERR and emit(base=None) == ERR and emit(stream=None) == ERR
    assert emit(F=0) == ERR and emit(B=0) == ERR and emit(B=8) == ERR
    assert emit(capacity=0) == ERR and emit(capacity=62) == ERR and emit(capacity=2 ** 32) == ERR and emit(stream=P + 1) == ERR
    assert (_lib.JPEG_DCT_THREADS, _lib.JPEG_THREADS, _lib.JPEG_MAX_BLOCK_BITS, _lib.JPEG_MAX_DIM) == (256, 256, 1664, 65535)
    assert mjpeg.MAX_BLOCK_BITS == _lib.JPEG_MAX_BLOCK_BITS and mjpeg.MAX_DIM == _lib.JPEG_MAX_DIM
    header = open(os.path.join(ROOT, "include", "stv.h")).read()
    for name, value in (("DCT_THREADS", 256), ("THREADS", 256), ("MAX_BLOCK_BITS", 1664), ("MAX_DIM", 65535)):
        assert f"#define STV_JPEG_{name} {value}\n" in header


def test_the_block_bound_holds_for_the_tables():
    """STV_JPEG_MAX_BLOCK_BITS: the longest DC code plus 11 value bits, and 63 times the longest AC code plus 10."""
    dc = max(n for table in jr.DC for _, n in table.values()) + 11
    ac = max(n for table in jr.AC for _, n in table.values()) + 10
    assert dc + 63 * ac <= mjpeg.MAX_BLOCK_BITS
    worst = np.full((6, 64), -1023, dtype=np.int16)
    worst[:, 0] = [1023, -1024, 1023, -1024, -1024, -1024]
    assert int(jr.block_bits(worst).max()) <= mjpeg.MAX_BLOCK_BITS
