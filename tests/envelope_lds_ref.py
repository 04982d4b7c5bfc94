"""The envelope stage's dynamic LDS byte counts as the host computed them before the kernel and the host shared
one layout function (csrc/dkg_device.h env_lds): test infrastructure, not a test.

The three functions are transcriptions of the former host formulas (envelope_lds_bytes, envelope_grad_lds_bytes,
envelope_grad_rows_lds_bytes of csrc/dkg_kernels.hip), term by term, with the helpers they called; nothing here is
derived from env_lds.  tests/test_envelope_lds_host.py holds the shared layout's totals to them.
"""

ENV_CAP = 128
HCAP = 128
STAGED_SLOTS = 8
LIST_CAP_STREAM = 512
VCAP = 64
VREG = 3 * VCAP
STAGE_FRONT = 8
DKG_MAX_DIM = 16
SIZEOF_DOUBLE = 8


def outputs_bucket(m):
    return 1 if m <= 1 else 2 if m <= 2 else 3 if m <= 3 else 4 if m <= 4 else 8


def cov_rec(m):
    return 1 if m <= 1 else 2 if m <= 2 else 4 if m <= 4 else 8


def env_slots(lines):
    return 2 if lines <= 64 * 2 else 8 if lines <= 64 * 8 else 17 if lines <= 64 * 17 else 33


def stream_staged(M):
    return 2 <= M <= 4


def staged_chunk_len(rec):
    return STAGED_SLOTS * 64 * rec


def list_cap(refine):
    return LIST_CAP_STREAM if refine else ENV_CAP


def stage_len(N):
    return ((N + 127) // 128) * 128


def stage_stride(N, rec):
    slots = 64 * env_slots(N + 1) * rec
    return max(stage_len(N * rec), slots) + STAGE_FRONT


def envelope_lds_bytes(m, N, waves, S, stream, grad=False):
    M = outputs_bucket(m)
    staged = 0 if stream else 2 * stage_stride(N, cov_rec(M))
    refine = stream and not grad
    lc = list_cap(refine)
    if not refine:
        vroom = 0
    elif stream_staged(M):
        vroom = max(waves * VREG, 4 * staged_chunk_len(cov_rec(M)))
    else:
        vroom = waves * VREG
    return (STAGE_FRONT + staged + ((S * m + 1) & ~1) + ((S + 1) & ~1) + waves * 2 * lc + vroom +
            (0 if grad else (waves * lc + 1) // 2)) * SIZEOF_DOUBLE


def envelope_grad_lds_bytes(m, N, waves, S, d, max_np, stream):
    M = outputs_bucket(m)
    extra = ((waves * ENV_CAP + 1) // 2 + M * stage_len(max_np) + M * d * stage_len(max_np) +
             2 * M * DKG_MAX_DIM + waves * 64 + DKG_MAX_DIM + M * DKG_MAX_DIM + waves * (HCAP + max_np + ENV_CAP) +
             (waves * HCAP + 1) // 2)
    return envelope_lds_bytes(m, N, waves, S, stream, True) + extra * SIZEOF_DOUBLE


def envelope_grad_rows_lds_bytes(m, N, waves, S, max_np):
    M = outputs_bucket(m)
    extra = ((waves * ENV_CAP + 1) // 2 + 2 * M * DKG_MAX_DIM + waves * 64 + DKG_MAX_DIM + M * DKG_MAX_DIM +
             waves * (HCAP + max_np + ENV_CAP) + (waves * HCAP + 1) // 2)
    return envelope_lds_bytes(m, N, waves, S, True, True) + extra * SIZEOF_DOUBLE
