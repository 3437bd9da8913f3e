"""The arm table of the BLSTM ring recurrence kernels (csrc/lstm_ring.hip), stated once on the host for the tests.

A chain of the ring is NW = ceil(H / 12) workgroups of 12 hidden units.  The two entry points choose a separately compiled kernel
from NW alone:

    ams_blstm_ring_fwd   lstm_ring_fwd_kernel<NR, ARITH>       NR  = ceil(NW / 4) in 1..7   (producer rounds per wave)
    ams_blstm_ring_bwd   lstm_ring_bwd_kernel<NI, NPG, ARITH>  arm = ceil(NW / 5) in 1..6   (NI = NPG = arm)

ARITH of the forward kernel: 0 = f32 MFMA (AMS_LSTM_RING_X6=0 only), 1 = bf16x6 (the default), 2 = fp16x3 (a bound of the recurrent
kernels is given); of the backward kernel: 0 = f32 MFMA, 2 = fp16x3.  21 + 12 instantiations.  Above H = 336 (NW = 28) no ring is
taken and the per-step kernels of csrc/lstm.hip run.

A plain helper module: no test, no fixture."""

UW = 12                 # hidden units per workgroup
RING_MAX_H = 336

FWD_ARITH = (0, 1, 2)
BWD_ARITH = (0, 2)


def nw(H):
    return (H + UW - 1) // UW


def takes_ring(H):
    return H <= RING_MAX_H


def fwd_arm(H):
    """NR of lstm_ring_fwd_kernel<NR, .>."""
    return (nw(H) + 3) // 4


def bwd_arm(H):
    """NI = NPG of lstm_ring_bwd_kernel<NI, NPG, .>."""
    return (nw(H) + 4) // 5


FWD_ARMS = tuple(range(1, 8))
BWD_ARMS = tuple(range(1, 7))

# last H of an arm | first H of the next (336 closes the last arm of both)
FWD_BOUNDARIES = ((48, 49), (96, 97), (144, 145), (192, 193), (240, 241), (288, 289))
BWD_BOUNDARIES = ((60, 61), (120, 121), (180, 181), (240, 241), (300, 301))

# Every first-of-arm size is 1 and every last-of-arm size is 0 (mod 12): one interior size per forward arm 2..7 whose last workgroup
# (H % 12), last granule (H % 3) and last group of four workgroups (NW % 4) are all partial.
INTERIOR = (77, 131, 170, 215, 262, 319)

H_CASES = tuple(sorted(set(h for pair in FWD_BOUNDARIES + BWD_BOUNDARIES for h in pair) | {RING_MAX_H} | set(INTERIOR)))
