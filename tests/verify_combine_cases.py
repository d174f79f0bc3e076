"""Shared by tests/test_gpu_verify_combine.py and its child processes: bursts of single-proof verify requests through the call
combiner (bbp_verify_async / bbp_verify), and the request sets the tests use.  A request is (record, score, z_img, seed, pub_list)."""
import json
import sys
import threading

L = 2 ** 252 + 27742317777372353535851937790883648493
NS_BURST = (1, 2, 3, 5, 8, 13, 40, 202)


def n_of(req):
    return len(req[4]) // 32


def two_phase(req):
    """The same proof in the two-phase R1CSProof layout: version byte 1, A_I2 = A_O2 = S2 = identity (tests/test_gpu_prove_verify.py)."""
    rec = req[0]
    return (b"\x01" + rec[1:97] + bytes(96) + rec[97:],) + tuple(req[1:])


def corrupt(req, kind):
    rec, score = bytearray(req[0]), bytearray(req[1])
    if kind == "bit":        # one bit of t_x_blinding's neighbourhood: a point or scalar of the proof changes
        rec[len(rec) // 3] ^= 0x04
    elif kind == "score":    # a wrong (still canonical) score
        score[0] ^= 0x01
    elif kind == "version":  # first byte neither 0 nor 1
        rec[0] = 7
    else:
        raise ValueError(kind)
    return (bytes(rec), bytes(score)) + tuple(req[2:])


def burst(handle, reqs, timeout=240.0):
    """Submit every request with bbp_verify_async, back to back from this thread; the statuses in request order."""
    out = [None] * len(reqs)
    left = [len(reqs)]
    lock, done = threading.Lock(), threading.Event()

    def finish(i, st):
        with lock:
            out[i] = st
            left[0] -= 1
            if left[0] == 0:
                done.set()
    keep = [handle.verify_async(*r, (lambda st, i=i: finish(i, st))) for i, r in enumerate(reqs)]
    assert done.wait(timeout), "verify_async callbacks missing: %d of %d" % (left[0], len(reqs))
    del keep
    return out


def to_json(reqs):
    return [[x.hex() for x in r] for r in reqs]


def from_json(rows):
    return [tuple(bytes.fromhex(x) for x in r) for r in rows]


def child_main(path_in, path_out):
    """Child process of the GPU tests (its environment carries what the test is about, e.g. BBP_VERIFY_AGGREGATE): one context,
    a 100 ms window, every burst of the input file; writes statuses, call counts and the engine's description."""
    try:
        import torch  # noqa: F401  (its HIP runtime first: tests/conftest.py)
    except ImportError:
        pass
    import dusk_blindbidproof_amd as bbp
    job = json.load(open(path_in))
    c = bbp.Context(0)
    if job.get("entropy"):
        c.set_entropy_source(job["entropy"])
    c.set_batching(100000, 4096)
    res = []
    for rows in job["bursts"]:
        before = c.batching_stats()
        st = burst(c, from_json(rows))
        after = c.batching_stats()
        res.append({"status": st, "calls": after[0] - before[0]})
    json.dump({"bursts": res, "describe": c.describe(), "health": c.health()}, open(path_out, "w"))
    c.close()


if __name__ == "__main__":
    child_main(sys.argv[1], sys.argv[2])
