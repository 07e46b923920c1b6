"""liblinear::LibLinearClassifier::loadStaticNegatives of the host layer on hand-written files: separators, maxNegatives, scale, a
missing file, and a row of the wrong length, which is std::invalid_argument at the training before any device is touched.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include "liblinear/LibLinearClassifier.hpp"
using liblinear::LibLinearClassifier;

int main(int argc, char** argv) {
    if (argc > 5) {   // train with the file's rows behind examples of argv[5] values: has to throw before a context is created
        LibLinearClassifier c(1.0, false);
        c.loadStaticNegatives(argv[1], std::atoi(argv[2]), std::atof(argv[3]));
        const int d = std::atoi(argv[5]);
        std::vector<cv::Mat> pos{cv::Mat::zeros(1, d, CV_32FC1)}, neg{cv::Mat::zeros(1, d, CV_32FC1)};
        try {
            c.retrain(pos, neg);
            std::printf("trained\n");
        } catch (const std::invalid_argument& e) {
            std::printf("invalid_argument %s\n", e.what());
        }
        return 0;
    }
    LibLinearClassifier c(1.0, argc > 4 && std::atoi(argv[4]) != 0);
    c.loadStaticNegatives(argv[1], std::atoi(argv[2]), std::atof(argv[3]));
    std::printf("rows %zu usable %d\n", c.getStaticNegatives().size(), c.isUsable() ? 1 : 0);
    for (const auto& row : c.getStaticNegatives()) {
        std::printf("row");
        for (float v : row) std::printf(" %.9g", v);
        std::printf("\n");
    }
    return 0;
}
'''

FILE = "1,2.5,-3\n4;5;6e-1\n7 8 -9\n 10 , 11 ,12 \n1,2,3,\n1 2\n13,14,15\n"
ROWS = [[1, 2.5, -3], [4, 5, 0.6], [7, 8, -9], [10, 11, 12], [1, 2, 3, 0], [1, 2], [13, 14, 15]]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("liblinear_host")
    src, exe = d / "negatives.cpp", d / "negatives"
    src.write_text(PROGRAM)
    pkg = os.path.join(ROOT, "featuredetection_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(pkg, "host", "include"), "-I",
                    os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", pkg, "-lfd_host", "-lfd_hip", "-Wl,-rpath," + pkg], check=True)
    (d / "negatives.txt").write_text(FILE)
    return str(exe), str(d / "negatives.txt")


def _rows(program, *args):
    run = subprocess.run([program[0]] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    rows = [np.array(l.split()[1:], np.float32) for l in lines[1:]]
    assert lines[0] == "rows %d usable 0" % len(rows)
    return rows


def test_separators_and_line_ends(program):
    """comma, semicolon and blanks separate; blanks around a separator are skipped; a separator at the end of the line is followed
    by the 0 of the failed read, as in the reference"""
    rows = _rows(program, program[1], 100, 1.0)
    assert len(rows) == len(ROWS)
    for got, want in zip(rows, ROWS):
        assert got.tobytes() == np.array(want, np.float32).tobytes()


def test_at_most_max_negatives_lines(program):
    assert len(_rows(program, program[1], 3, 1.0)) == 3
    assert len(_rows(program, program[1], 0, 1.0)) == 0


def test_scale_is_applied_in_double_then_rounded(program):
    rows = _rows(program, program[1], 2, 0.1)
    want = [[np.float32(0.1 * v) for v in r] for r in ROWS[:2]]
    for got, w in zip(rows, want):
        assert got.tobytes() == np.array(w, np.float32).tobytes()


def test_the_bias_flag_does_not_change_the_stored_rows(program):
    """the constant-1 feature is implicit on the device"""
    assert [r.tobytes() for r in _rows(program, program[1], 4, 1.0, 1)] == [r.tobytes() for r in _rows(program, program[1], 4, 1.0, 0)]


def test_a_missing_file_yields_nothing(program):
    assert _rows(program, program[1] + ".missing", 10, 1.0) == []


def test_a_row_of_the_wrong_length_is_refused_at_the_training(program):
    run = subprocess.run([program[0], program[1], "5", "1.0", "0", "3"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    assert run.stdout.startswith("invalid_argument LibLinearClassifier: a static negative example has 4 values, the examples 3")


def test_host_header_compiles():
    inc = os.path.join(ROOT, "featuredetection_amd", "host", "include")
    src = '#include "liblinear/LibLinearClassifier.hpp"\nint main() { return 0; }\n'
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", inc, "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"], input=src.encode(),
                   check=True)
