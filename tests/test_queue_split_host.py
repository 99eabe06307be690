"""CPU test of the two-ended chunk queue's index arithmetic (csrc/nddm_queue.h: queue_pull), compiled for the host the way the
tools/*_host.py programs compile the headers of csrc/: random interleavings of front and back pullers, each pulling until it has seen
the queue dry once, hand out every chunk exactly once and nothing after the counts have reached n_chunks."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import host_build  # noqa: E402

MAIN = r"""// usage: queue_host in.bin out.bin ; in: int32 n_chunks, int32 n_pulls, then n_pulls bytes (0 = a front pull, 1 = a back pull), in the
// order in which the atomic adds reach the queue word; out: int64 per pull, the chunk or -1
#include <cstdio>
#include <vector>
#include "nddm_queue.h"
int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb"); int hdr[2]; if (!f || fread(hdr, 4, 2, f) != 2) return 2;
    std::vector<unsigned char> ends((size_t)hdr[1]);
    if (hdr[1] && fread(ends.data(), 1, ends.size(), f) != ends.size()) return 3;
    fclose(f);
    std::vector<long long> out(ends.size());
    unsigned long long word = 0;                                   // the queue word: zero between launches
    for (size_t i = 0; i < ends.size(); ++i) {
        const unsigned long long old = word;                       // what the atomic add returns
        word += ends[i] ? nddm::QUEUE_BACK : nddm::QUEUE_FRONT;
        out[i] = nddm::queue_pull(old, hdr[0], ends[i] != 0);
    }
    f = fopen(argv[2], "wb"); if (!f) return 4;
    fwrite(out.data(), 8, out.size(), f); fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def queue_host():
    with tempfile.TemporaryDirectory() as td:
        exe = host_build.build(td, MAIN, "queue_host")

        def pull(n_chunks, ends):
            ends = np.asarray(ends, np.uint8)
            with open(os.path.join(td, "in.bin"), "wb") as f:
                f.write(np.array([n_chunks, len(ends)], np.int32).tobytes())
                f.write(ends.tobytes())
            subprocess.check_call([exe, os.path.join(td, "in.bin"), os.path.join(td, "out.bin")])
            return np.fromfile(os.path.join(td, "out.bin"), np.int64)
        yield pull


def interleaving(rng, n_chunks, n_front, n_back):
    """The pulls of n_front + n_back pullers in a random order: every puller keeps pulling until it has seen "dry" once (the first n_chunks
    pulls of the whole sequence are the valid ones, whoever makes them).  Picks the next puller uniformly or with a random bias towards one
    end, as a grid whose front waves are faster has it."""
    ends = np.array([0] * n_front + [1] * n_back, np.uint8)
    alive = list(range(len(ends)))
    weight = np.where(ends == 0, rng.choice([0.1, 1.0, 10.0]), 1.0)
    seq = []
    while alive:
        w = weight[alive]
        i = alive[rng.choice(len(alive), p=w / w.sum())]
        if len(seq) >= n_chunks:                                   # this pull finds the queue dry: the puller is done
            alive.remove(i)
        seq.append(ends[i])
    return np.array(seq, np.uint8)


@pytest.mark.parametrize("n_chunks", [1, 2, 3, 7, 1000])
def test_every_chunk_comes_out_exactly_once(queue_host, n_chunks):
    rng = np.random.default_rng(20 + n_chunks)
    for n_front, n_back in [(1, 1), (3, 1), (1, 3), (5, 5), (48, 16), (0, 4), (4, 0)] * 3:
        ends = interleaving(rng, n_chunks, n_front, n_back)
        assert len(ends) == n_chunks + n_front + n_back            # every puller sees "dry" exactly once
        got = queue_host(n_chunks, ends)
        valid = got >= 0
        assert valid[:n_chunks].all() and not valid[n_chunks:].any()          # nothing after the counts reach n_chunks
        assert sorted(got[valid].tolist()) == list(range(n_chunks))           # every chunk, exactly once
        front, back = got[valid & (ends == 0)], got[valid & (ends == 1)]
        assert front.tolist() == list(range(len(front)))                      # 0, 1, 2, ... from the front
        assert back.tolist() == list(range(n_chunks - 1, n_chunks - 1 - len(back), -1))   # n - 1, n - 2, ... from the back


@pytest.mark.parametrize("n_chunks", [1, 2, 3, 7, 1000])
def test_an_all_front_sequence_is_the_one_ended_queue(queue_host, n_chunks):
    got = queue_host(n_chunks, np.zeros(n_chunks + 9, np.uint8))
    assert got.tolist() == list(range(n_chunks)) + [-1] * 9


def test_the_header_is_part_of_the_source_hash_and_the_knob_is_exported():
    from bayesflow_nddms_amd import _lib, build
    assert any(p.endswith("nddm_queue.h") for p in build.HEADERS)
    assert "nddm_set_queue_split" in _lib.EXPORTS
    assert "int nddm_set_queue_split(int back_waves);" in open(os.path.join(ROOT, "include", "nddm.h")).read()
