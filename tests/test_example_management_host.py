"""The example stores of the host layer (classification::AgeBasedExampleManagement, ConfidenceBasedExampleManagement,
UnlimitedExampleManagement, EmptyExampleManagement): a small program on the host headers plays seeded `add` sequences and
prints the stores' contents, which are compared with a Python restatement of AgeBasedExampleManagement.cpp:18-30 and
ConfidenceBasedExampleManagement.cpp:28-68 -- capacity, wrap-around, `keep`, and the replacement order with a stub classifier.
No device is involved."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include "classification/AgeBasedExampleManagement.hpp"
#include "classification/ConfidenceBasedExampleManagement.hpp"
#include "classification/EmptyExampleManagement.hpp"
#include "classification/UnlimitedExampleManagement.hpp"
using namespace classification;

// examples are 1 x 1 float matrices holding an id; the stub's signed score of an id comes from a table
struct Stub : BinaryClassifier {
    std::map<int, double> score;
    bool classify(const cv::Mat& m) const override { return getConfidence(m).first; }
    std::pair<bool, double> getConfidence(const cv::Mat& m) const override {
        const double s = score.at((int)m.at<float>(0, 0));
        return std::make_pair(s >= 0, s >= 0 ? s : -s);
    }
};

static void print(const ExampleManagement& store) {
    std::printf("%zu %d :", store.size(), store.hasRequiredSize() ? 1 : 0);
    for (auto it = store.iterator(); it->hasNext();) std::printf(" %d", (int)it->next().at<float>(0, 0));
    std::printf("\n");
}

int main() {
    auto stub = std::make_shared<Stub>();
    std::unique_ptr<ExampleManagement> store;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        in >> op;
        if (op == "store") {
            std::string kind;
            size_t capacity, required, keep;
            in >> kind >> capacity >> required >> keep;
            if (kind == "age") store.reset(new AgeBasedExampleManagement(capacity, required));
            else if (kind == "unlimited") store.reset(new UnlimitedExampleManagement(required));
            else if (kind == "empty") store.reset(new EmptyExampleManagement());
            else {
                auto c = new ConfidenceBasedExampleManagement(stub, kind == "confpos", capacity, required);
                if (keep != 1) c->setFirstExamplesToKeep(keep);   // 1 is the default
                store.reset(c);
            }
        } else if (op == "add") {
            std::vector<cv::Mat> examples;
            int id;
            double score;
            while (in >> id >> score) {
                cv::Mat m(1, 1, CV_32FC1);
                m.at<float>(0, 0) = (float)id;
                stub->score[id] = score;
                examples.push_back(m);
            }
            store->add(examples);
            print(*store);
        } else if (op == "clear") {
            store->clear();
            print(*store);
        }
    }
    try {
        EmptyExampleManagement().iterator()->next();
        std::printf("no exception\n");
    } catch (const std::runtime_error&) {
        std::printf("runtime_error\n");
    }
    return 0;
}
'''


class Store:
    """the Python restatement: ids in storage order"""

    def __init__(self, kind, capacity, required, keep):
        self.kind, self.capacity, self.required, self.keep = kind, capacity, required, keep
        self.ids, self.insert, self.score = [], 0, {}
        if kind == "unlimited":
            self.capacity = None

    def conf(self, i):
        return self.score[i] if self.kind == "confpos" else -self.score[i]

    def add(self, new):
        for i, s in new:
            self.score[i] = s
        new = [i for i, _ in new]
        if self.kind == "empty":
            return
        if self.kind == "unlimited":
            self.ids += new
        elif self.kind == "age":
            for i in new:
                if len(self.ids) < self.capacity:
                    self.ids.append(i)
                else:
                    self.ids[self.insert] = i
                    self.insert = (self.insert + 1) % len(self.ids)
        else:
            existing = sorted(range(self.keep, len(self.ids)), key=lambda p: -self.conf(self.ids[p]))   # most confident first
            incoming = sorted(new, key=self.conf)                                                      # least confident first
            while len(self.ids) < self.capacity and incoming:
                self.ids.append(incoming.pop(0))
            for p in existing:
                if not incoming or not self.conf(incoming[0]) < self.conf(self.ids[p]):
                    break
                self.ids[p] = incoming.pop(0)

    def clear(self):
        self.ids = []   # the insert position stays, as in the reference

    def line(self):
        return "%d %d :%s" % (len(self.ids), 1 if self.kind == "empty" or len(self.ids) >= self.required else 0,
                              "".join(" %d" % i for i in self.ids))


def _script():
    """stores and add sequences: under, at and over the capacity, several wraps, batches larger than the capacity, empty batches,
    clear in the middle; distinct scores (the order of equal confidences is the sort's)"""
    rng = np.random.default_rng(20261018)
    next_id = [0]
    scores = rng.permutation(4000) / 1000.0 - 2.0   # distinct, both signs

    def batch(n):
        out = []
        for _ in range(n):
            out.append((next_id[0], float(scores[next_id[0]])))
            next_id[0] += 1
        return out

    ops = []
    stores = [("age", 4, 1, 1), ("age", 5, 3, 1), ("age", 1, 1, 1), ("unlimited", 0, 12, 1), ("empty", 0, 0, 1),
              ("confpos", 5, 2, 1), ("confneg", 5, 2, 1), ("confpos", 6, 1, 0), ("confneg", 6, 1, 3), ("confpos", 3, 1, 5), ("confneg", 20, 1, 1)]
    for st in stores:
        ops.append(("store",) + st)
        for n in [1, 2, 0, 3, 1, 7, 2, 13, 1, 1, 4]:
            ops.append(("add", batch(n)))
        ops.append(("clear",))
        for n in [2, 9, 3]:
            ops.append(("add", batch(n)))
    return ops


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("example_management")
    src, exe = d / "stores.cpp", d / "stores"
    src.write_text(PROGRAM)
    pkg = os.path.join(ROOT, "featuredetection_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(pkg, "host", "include"), "-I",
                    os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", pkg, "-lfd_host", "-lfd_hip", "-Wl,-rpath," + pkg], check=True)
    return str(exe)


def test_add_sequences_equal_the_restatement(program):
    ops = _script()
    text, want, store = [], [], None
    for op in ops:
        if op[0] == "store":
            text.append("store %s %d %d %d" % op[1:])
            store = Store(*op[1:])
        elif op[0] == "add":
            text.append("add" + "".join(" %d %r" % e for e in op[1]))
            store.add(op[1])
            want.append(store.line())
        else:
            text.append("clear")
            store.clear()
            want.append(store.line())
    run = subprocess.run([program], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got = run.stdout.splitlines()
    assert got[-1] == "runtime_error"   # EmptyExampleManagement's iterator has nothing to return
    assert len(got) - 1 == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)


def test_restatement_on_known_sequences():
    """the restatement itself, by hand: the ring of the age-based store and the replacement order of the confidence-based one"""
    s = Store("age", 3, 1, 1)
    s.add([(1, 0), (2, 0)])
    s.add([(3, 0), (4, 0)])          # 4 overwrites the oldest
    assert s.ids == [4, 2, 3]
    s.add([(5, 0), (6, 0), (7, 0), (8, 0)])   # a batch larger than the capacity wraps
    assert s.ids == [7, 8, 6]
    c = Store("confpos", 3, 1, 1)
    c.add([(1, 0.9), (2, 0.5), (3, 0.7)])     # free space is filled least confident first
    assert c.ids == [2, 3, 1]
    c.add([(4, 0.1), (5, 0.8), (6, 0.2)])     # 4 replaces the most confident replaceable (1), 6 the next (3); 2 is kept (keep = 1)
    assert c.ids == [2, 6, 4]
    n = Store("confneg", 2, 1, 0)
    n.add([(1, -0.9), (2, 0.3)])              # a negative store trusts negative scores: 2 is the less confident
    assert n.ids == [2, 1]
    n.add([(3, 0.5)])                         # replaces 1, the most confident negative
    assert n.ids == [2, 3]
