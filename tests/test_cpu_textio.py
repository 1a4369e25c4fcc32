"""What the text readers share on the host (snprelate_amd/textio.py) and the staging windows of the text calls
(snprelate_amd/csrc/text_windows.h), each on its own: no device, no library."""
import io
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from snprelate_amd import textio


# ---- the chunk loop ------------------------------------------------------------------------------------------------------------------
def _text(final_newline):
    """about 40 lines of 0, 1 and up to 30 bytes"""
    rng = np.random.default_rng(11)
    lengths = [0, 1, 30, 0, 0, 1, 29] + [int(x) for x in rng.integers(0, 31, 34)]
    lines = [bytes(rng.integers(0x41, 0x5B, k, dtype=np.uint8)) for k in lengths]
    lines[-1] = lines[-1] or b"Z"                          # a last line without a line end is a line only when it has bytes
    return b"\n".join(lines) + (b"\n" if final_newline else b""), lines


def _read(text, size, env_name="SNPGPU_SOME_BYTES"):
    """the lines and the `final` of every chunk of `text` read with two buffers of `size` bytes"""
    buffers = [np.zeros(size, np.uint8) for _ in range(2)]
    index = lambda buf, n, final: textio.split_lines(buf, n, final, strip_cr=False)         # noqa: E731
    lines, finals = [], []
    for buf, n, final, begin, end in textio.chunks(io.BytesIO(text), buffers, index, "some.txt", env_name):
        assert any(buf is b for b in buffers) and 0 < n <= size and len(begin) == len(end)
        assert final == (n < size)                         # the rule: a chunk that fills its buffer is not known to be the last
        lines += [bytes(buf[b:e]) for b, e in zip(begin, end)]
        finals.append(final)
    return lines, finals


@pytest.mark.parametrize("final_newline", [True, False])
def test_chunks_give_every_line_once_in_order(final_newline):
    text, want = _text(final_newline)
    assert want == (text.split(b"\n")[:-1] if final_newline else text.split(b"\n")) and 30 in map(len, want) and b"" in want
    longest = max(len(x) for x in want)
    full_ends = 0
    for size in range(longest + 1, len(text) + 2):
        lines, finals = _read(text, size)
        assert lines == want, size
        # `final` is true on the last chunk and on no other -- but for a last chunk whose whole lines fill the buffer to its end
        assert not any(finals[:-1]), size
        if not final_newline:
            assert finals[-1], size
        if size == len(text):
            assert finals == ([False] if final_newline else [False, True])
        if size > len(text):
            assert finals == [True]
        full_ends += not finals[-1]
    assert (full_ends >= 1) if final_newline else (full_ends == 0)


@pytest.mark.parametrize("final_newline", [True, False])
def test_a_line_longer_than_a_chunk_is_refused_by_the_name_passed_in(final_newline):
    text, want = _text(final_newline)
    longest = max(len(x) for x in want)
    for size in (longest, longest - 1, 1):
        with pytest.raises(ValueError) as e:
            _read(text, size, "SNPGPU_OTHER_BYTES")
        assert str(e.value) == "'some.txt': a line longer than the %d bytes of a chunk (SNPGPU_OTHER_BYTES)" % size


def test_an_empty_file_has_no_chunk():
    assert _read(b"", 8) == ([], [])


def test_split_lines_with_and_without_cr():
    buf = np.frombuffer(b"a\r\nb\n\r\n", np.uint8)
    begin, end, used = textio.split_lines(buf, len(buf), True, strip_cr=False)
    assert begin.tolist() == [0, 3, 5] and end.tolist() == [2, 4, 6] and used == 7
    begin, end, used = textio.split_lines(buf, len(buf), True, strip_cr=True)
    assert begin.tolist() == [0, 3, 5] and end.tolist() == [1, 4, 5] and used == 7          # the lone '\r': end == begin, not below
    # an empty line behind a line that ends in '\r' is not stripped into it
    buf = np.frombuffer(b"\r\n\nab", np.uint8)
    begin, end, used = textio.split_lines(buf, len(buf), False, strip_cr=True)
    assert begin.tolist() == [0, 2] and end.tolist() == [0, 2] and used == 3                 # the cut line "ab" is left
    begin, end, used = textio.split_lines(buf, len(buf), True, strip_cr=True)
    assert begin.tolist() == [0, 2, 3] and end.tolist() == [0, 2, 5] and used == 5
    begin, end, used = textio.split_lines(buf, 0, True, strip_cr=True)
    assert len(begin) == 0 and len(end) == 0 and used == 0


# ---- the staging windows -------------------------------------------------------------------------------------------------------------
def test_window_planner_against_brute_force(tmp_path):
    """tests/text_windows_check.cpp includes only text_windows.h; built with the host compiler under the address and
    undefined-behaviour sanitizers and run as a process of its own, it prints nothing and exits 0"""
    exe = str(tmp_path / "text_windows_check")
    r = subprocess.run(["g++", "-std=gnu++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "snprelate_amd", "csrc"), os.path.join(ROOT, "tests", "text_windows_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == "" and r.stderr == "", (r.stdout + r.stderr)[-3000:]
