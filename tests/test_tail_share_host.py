"""not-gpu tier: the IPA tail's walk with the B-term share on the CPU (tests/tail_share_check.cpp compiles csrc/scalarmul.h's
ge_scalarmul_pieces_shared and tail_share_of under AddressSanitizer + UBSan, nothing preloaded).  One side of k_tail_lr's wavefront --
32 lanes, each with its own term and two of the 64 digits of c w -- must sum to the 32 terms plus (c w) B, for the B scalars at the
recoding's edges and for term scalars at zero."""
import subprocess


def test_side_sum_with_the_b_share_equals_terms_plus_b(built):
    r = subprocess.run([built.build_tail_share_check()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "tail_share_check ok" in r.stdout, r.stdout[-400:] + r.stderr[-2000:]
