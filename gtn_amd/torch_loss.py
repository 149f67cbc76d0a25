"""PyTorch entry points of the hot path: `ctc_loss`, `asg_loss`, `ctc_forced_align`,
`asg_forced_align`, `asg_decode`, `ctc_decode`, `ctc_sample`, `ctc_beam_decode`, `asg_beam_decode`, `asg_sample`,
`edit_distance`, `ctc_score`, `ctc_lattice_score`, `ctc_lattice_loss`, `ctc_lattice_align`, `ctc_token_align`,
`asg_score`, `asg_lattice_score`, `asg_full_connect`, `asg_lattice_loss` and `asg_token_align`.

`ctc_loss` is the device-resident counterpart of the reference's
bindings/python/examples/pytorch_loss.py:19-102: the emissions tensor never leaves
the GPU (no inputs.cpu(), no per-sample weights_to_numpy), the batch runs through
the batched graph functions, and the emission gradients come back as one tensor.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

import gtn_amd as gtn

_NATIVE = None


_P, _I, _F = C.c_void_p, C.c_int, C.c_float
# the argument types of libgtn_criteria.so's entry points (gtn_amd/criteria/criteria_capi.cpp); all return an int.  A
# library from before an entry point lacks its symbol
_ARGTYPES = {
    "gtn_ctc_loss_n": [_P, _P, _P, _I, _I, _I, _I, _P, _P],
    "gtn_ctc_loss_frames_n": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P],
    "gtn_asg_loss_n": [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P],
    "gtn_asg_loss_frames_n": [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P],
    "gtn_ctc_align_n": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P],
    "gtn_asg_align_n": [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P],
    "gtn_asg_decode_n": [_P, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    "gtn_ctc_decode_n": [_P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    "gtn_ctc_sample_n": [_P, _I, _I, _I, _I, _P, _I, C.c_uint64, _F, _P, _P, _P, _P],
    "gtn_ctc_beam_decode_n": [_P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _P, _P],
    "gtn_ctc_beam_decode_lm_n": [_P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _F, _F, _P, _P, _P, _P],
    "gtn_ctc_beam_decode_graph_n": [_P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _F, _F, _P, _P, _P, _P],
    "gtn_edit_distance_n": [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P],
    "gtn_ctc_score_n": [_P, _I, _I, _I, _I, _P, _P, _P, _I, _I, _I, _P],
    "gtn_ctc_score_grad_n": [_P, _I, _I, _I, _I, _P, _P, _P, _I, _I, _I, _P, _P],
    "gtn_ctc_lattice_score_n": [_P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _I, _P],
    "gtn_ctc_lattice_score_grad_n": [_P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P],
    "gtn_ctc_lattice_align_n": [_P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P],
    "gtn_ctc_token_align_n": [_P, _I, _I, _I, _I, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P],
    "gtn_asg_score_n": [_P, _I, _I, _I, _P, _P, _P, _P, _I, _I, _I, _P],
    "gtn_asg_score_grad_n": [_P, _I, _I, _I, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P],
    "gtn_asg_lattice_score_n": [_P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "gtn_asg_lattice_score_grad_n": [_P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P],
    "gtn_asg_full_connect_n": [_P, _I, _I, _I, _P, _P, _P, _P, _P],
    "gtn_asg_beam_decode_n": [_P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P],
    "gtn_asg_sample_n": [_P, _I, _I, _I, _P, _P, _I, C.c_uint64, _F, _P, _P, _P, _P, _P],
    "gtn_asg_beam_decode_graph_n": [_P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _F, _F, _P, _P, _P, _P],
    "gtn_asg_token_align_n": [_P, _I, _I, _I, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P],
}


def _native():
    """libgtn_criteria.so (gtn_amd/criteria/): the whole batch step in one native call --
    target graphs on host threads, batched graph functions, loss and gradient on the device"""
    global _NATIVE
    if _NATIVE is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libgtn_criteria.so")
        if os.path.exists(path) and not os.environ.get("GTN_AMD_PYTHON_CRITERIA"):
            lib = C.CDLL(path)
            lib.gtn_criteria_last_error.restype = C.c_char_p
            for name, argtypes in _ARGTYPES.items():
                if hasattr(lib, name):
                    getattr(lib, name).argtypes = argtypes
                    getattr(lib, name).restype = C.c_int
            _NATIVE = lib
        else:
            _NATIVE = False
    return _NATIVE


def _call(name, *args):
    """one entry point of libgtn_criteria.so; its error as a RuntimeError"""
    lib = _native()
    if getattr(lib, name)(*args) != 0:
        raise RuntimeError(lib.gtn_criteria_last_error().decode())


def _has_native(who, symbol, python_route=False):
    """whether `who` runs through `symbol` of libgtn_criteria.so.  Without the library it takes the Python route; so does
    an entry with `python_route` when the library is from before the symbol, where the others raise"""
    lib = _native()
    if lib and not hasattr(lib, symbol) and not python_route:
        raise RuntimeError(f"{who} needs {symbol} in gtn_amd/lib/libgtn_criteria.so (run __graft_entry__.build())")
    return bool(lib) and hasattr(lib, symbol)


def _ptr(t):
    """device address of an optional tensor"""
    return t.data_ptr() if t is not None else None


def _host_ptr(a):
    """host address of an optional numpy array"""
    return a.ctypes.data if a is not None else None


def _engine_stream(device):
    """point the engine at the caller's stream; returns the stream"""
    stream = torch.cuda.current_stream(device)
    gtn.set_stream(stream.cuda_stream if stream.cuda_stream else None)
    if not stream.cuda_stream:
        stream.synchronize()  # engine runs on its own stream
    return stream


def _engine_done(stream):
    """the tail of _engine_stream: on the null stream the caller's next kernel must wait for the engine's own stream"""
    if not stream.cuda_stream:
        gtn.synchronize()


def _route(stream, x, native, symbol, args, method, *margs, **mkw):
    """the tail of a device-output function over the slabs x [B, T, C]: where `native` says so `symbol` of
    libgtn_criteria.so with (x, B, T, C, *args), else `method` of the linear batch that borrows x; then _engine_done"""
    if native:
        _call(symbol, x.data_ptr(), *x.shape, *args)
    else:
        getattr(gtn.Batch.linear(*x.shape, x, calc_grad=False, borrow=True), method)(*margs, **mkw)
    _engine_done(stream)


def _asg_weights(start, transitions):
    """[N + N*N] in the arc order of gtn::criteria::asgTransitions: N start arcs, then arc N + i*N + j = j -> i"""
    return torch.cat([start.detach().reshape(-1), transitions.detach().reshape(-1)]).to(torch.float32).contiguous()


def ctc_target_graph(target, blank=0):
    """the target acceptor of benchmarks/ctc.cpp:40-58 / pytorch_loss.py's criterion"""
    L = 2 * len(target) + 1
    g = gtn.Graph(False)
    for l in range(L):
        idx = (l - 1) // 2
        g.add_node(l == 0, l == L - 1 or l == L - 2)
        label = target[idx] if l % 2 else blank
        g.add_arc(l, l, label)
        if l > 0:
            g.add_arc(l - 1, l, label)
        if l % 2 and l > 1 and label != target[idx - 1]:
            g.add_arc(l - 2, l, label)
    g.arc_sort()
    return g


class _CTCLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_probs, targets, blank, reduction, frames=None):
        assert log_probs.is_cuda and log_probs.dtype == torch.float32 and log_probs.dim() == 3
        B, T, C = log_probs.shape
        if len(targets) != B:
            raise ValueError(f"ctc_loss: {len(targets)} target sequences for a batch of {B}")
        ctx.ragged = frames is not None
        if frames is not None:
            return _CTCLoss._forward_frames(ctx, log_probs, targets, blank, reduction, frames)
        x = log_probs.contiguous()
        stream = torch.cuda.current_stream(x.device)
        gtn.set_stream(stream.cuda_stream if stream.cuda_stream else None)
        if not stream.cuda_stream:
            torch.cuda.current_stream(x.device).synchronize()  # engine runs on its own stream
        lib = _native()
        if lib:
            flat, lens = _flat_targets(targets)
            out = torch.empty(B, dtype=torch.float32, device=x.device)
            grad = torch.empty(B, T, C, dtype=torch.float32, device=x.device) if log_probs.requires_grad else None
            rc = lib.gtn_ctc_loss_n(x.data_ptr(), flat.ctypes.data, lens.ctypes.data, B, T, C, int(blank),
                                    out.data_ptr(), grad.data_ptr() if grad is not None else None)
            if rc != 0:
                raise RuntimeError(lib.gtn_criteria_last_error().decode())
            if not stream.cuda_stream:
                gtn.synchronize()
            ctx.graphs = None
            ctx.grad = grad
            ctx.shape = (B, T, C)
            ctx.reduction = reduction
            return out.mean() if reduction == "mean" else (out.sum() if reduction == "sum" else out)
        ems = gtn.linear_graph_n(B, T, C, x, calc_grad=log_probs.requires_grad)
        tgs = [ctc_target_graph(list(t), blank) for t in targets]
        losses = gtn.subtract(gtn.forward_score(ems), gtn.forward_score(gtn.intersect(tgs, ems)))
        out = torch.empty(B, dtype=torch.float32, device=x.device)
        gtn.items_to_device(losses, out)
        if not stream.cuda_stream:
            gtn.synchronize()
        ctx.graphs = (losses, ems)
        ctx.shape = (B, T, C)
        ctx.reduction = reduction
        if reduction == "mean":
            return out.mean()
        if reduction == "sum":
            return out.sum()
        return out

    @staticmethod
    def _forward_frames(ctx, log_probs, targets, blank, reduction, frames):
        """a padded batch: utterance b has frames[b] <= T frames (the pad rows are never read, their gradient is 0)"""
        B, T, C = log_probs.shape
        x = log_probs.contiguous()
        stream = torch.cuda.current_stream(x.device)
        gtn.set_stream(stream.cuda_stream if stream.cuda_stream else None)
        if not stream.cuda_stream:
            torch.cuda.current_stream(x.device).synchronize()  # engine runs on its own stream
        out = torch.empty(B, dtype=torch.float32, device=x.device)
        lib = _native()
        ctx.shape = (B, T, C)
        ctx.reduction = reduction
        if lib:
            if not hasattr(lib, "gtn_ctc_loss_frames_n"):
                raise RuntimeError("ctc_loss(input_lengths=...) needs gtn_ctc_loss_frames_n in "
                                   "gtn_amd/lib/libgtn_criteria.so (run __graft_entry__.build())")
            flat, lens = _flat_targets(targets)
            grad = torch.empty(B, T, C, dtype=torch.float32, device=x.device) if log_probs.requires_grad else None
            rc = lib.gtn_ctc_loss_frames_n(x.data_ptr(), flat.ctypes.data, lens.ctypes.data, B, T, C, int(blank),
                                           frames.ctypes.data, out.data_ptr(),
                                           grad.data_ptr() if grad is not None else None)
            if rc != 0:
                raise RuntimeError(lib.gtn_criteria_last_error().decode())
            ctx.graphs = None
            ctx.grad = grad
        else:
            ctcs = gtn.Batch.ctc_targets([list(t) for t in targets], blank, calc_grad=False)
            ems = gtn.Batch.linear(B, T, C, x, calc_grad=log_probs.requires_grad, borrow=True, rows=frames)
            # (this order lets the sweep over target o emissions leave forwardScore(emissions) behind)
            score = gtn.forward_score(gtn.intersect(ctcs, ems))
            losses = gtn.subtract(gtn.forward_score(ems), score)
            losses.items_to_device(out)
            ctx.graphs = (losses, ems)
            ctx.keep = x  # (borrowed by `ems` until the backward pass)
        if not stream.cuda_stream:
            gtn.synchronize()
        return out.mean() if reduction == "mean" else (out.sum() if reduction == "sum" else out)

    @staticmethod
    def backward(ctx, grad_out):
        B, T, C = ctx.shape
        if ctx.graphs is None:
            grad = ctx.grad  # computed with the forward pass by the native criterion
        elif isinstance(ctx.graphs[1], gtn.Batch):
            losses, ems = ctx.graphs
            gtn.backward(losses)
            grad = torch.empty(B, T, C, dtype=torch.float32, device=grad_out.device)
            ems.grads_to_device(grad, [b * T * C for b in range(B)])
            gtn.synchronize()
        else:
            losses, ems = ctx.graphs
            gtn.backward(losses)
            grad = torch.empty(B, T, C, dtype=torch.float32, device=grad_out.device)
            gtn.grads_to_device(ems, grad, [b * T * C for b in range(B)])
            gtn.synchronize()
        if ctx.reduction == "mean":
            scale = (grad_out / B).reshape(1, 1, 1)
        elif ctx.reduction == "sum":
            scale = grad_out.reshape(1, 1, 1)
        else:
            scale = grad_out.reshape(B, 1, 1)
        return (grad * scale, None, None, None) + ((None,) if ctx.ragged else ())


def _frame_counts(name, input_lengths, B, T, low):
    """per-utterance frame counts as a host int32 array [B], each in low .. T (low None: the engine checks the range)"""
    vals = input_lengths.tolist() if hasattr(input_lengths, "tolist") else list(input_lengths)
    frames = np.ascontiguousarray([int(v) for v in vals], dtype=np.int32)
    if frames.shape != (B,):
        raise ValueError(f"{name}: {frames.size} input lengths for a batch of {B}")
    if B and low is not None and (int(frames.min()) < low or int(frames.max()) > T):
        raise ValueError(f"{name}: an input length outside {low} .. {T}")
    return frames


def _hypothesis_args(who, computed, x, x_name, tokens, lengths, blank, input_lengths, max_length, own_checks=None):
    """What `ctc_score`, `asg_score`, `ctc_token_align` and `asg_token_align` check and normalise alike.  `x`: the emissions, `x_name` in
    the texts; `computed`: what the texts say the device computes; `blank`: None where there is none; `own_checks(C)`:
    the caller's own value checks, which return the (tensor or None, name) pairs that have to be on x's device as well.
    Returns (B, T, C, N, L, flat, tok, ln, frames, max_length): `flat` says tokens was [B, L]; tok is int32 [B, N, L]
    with an address, ln int32 [B, N], frames the host counts or None."""
    if not (torch.is_tensor(x) and x.dim() == 3 and x.dtype == torch.float32):
        raise ValueError(f"{who}: {x_name} must be a float32 tensor [B, T, C]")
    B, T, C_ = x.shape
    if not (torch.is_tensor(tokens) and tokens.dtype == torch.int32 and tokens.dim() in (2, 3) and tokens.shape[0] == B):
        raise ValueError(f"{who}: tokens must be an int32 tensor [B, N, L] or [B, L] for a batch of {B}")
    flat = tokens.dim() == 2
    N, L = (1, tokens.shape[1]) if flat else tokens.shape[1:]
    shape = (B,) if flat else (B, N)
    if not (torch.is_tensor(lengths) and lengths.dtype in (torch.int32, torch.int64) and tuple(lengths.shape) == shape):
        raise ValueError(f"{who}: lengths must be an int32 or int64 tensor {list(shape)}")
    if blank is not None and not 0 <= blank < C_:
        raise ValueError(f"{who}: blank must be one of the {C_} labels")
    max_length = max(1, min(L, T, 4096)) if max_length is None else int(max_length)
    if not 1 <= max_length <= 4096:
        raise ValueError(f"{who}: max_length outside 1 .. 4096")
    frames = None if input_lengths is None else _frame_counts(who, input_lengths, B, T, 0)
    more = own_checks(C_) if own_checks else ()
    for t, what in ((x, x_name), *more, (tokens, "tokens"), (lengths, "lengths")):
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"{who}: {what} must be a CUDA tensor (the {computed} are computed on the device)")
        if t.device != x.device:
            raise ValueError(f"{who}: all tensors must be on one device")
    tok = tokens.detach().reshape(B, N, L).contiguous()
    if B * N and tok.numel() == 0:
        tok = tok.new_empty(B, N, 1)[:, :, :0]  # (rows without an element are never read, but they need an address)
    ln = lengths.detach().to(torch.int32).reshape(B, N).contiguous()  # (int64 lengths are converted on the device)
    return B, T, C_, N, L, flat, tok, ln, frames, max_length


def ctc_loss(log_probs, targets, blank=0, reduction="none", input_lengths=None):
    """log_probs: float32 CUDA tensor [B, T, C] (any scores; the loss carries its own
    normaliser forwardScore(emissions), as in benchmarks/ctc.cpp:150-158).
    targets: sequence of B label sequences.  input_lengths: a sequence or int tensor of B frame
    counts (1 .. T) for a padded batch, or None: utterance b's loss is that of log_probs[b, :T_b]
    (+inf when its target does not fit into T_b frames), rows past T_b are never read and their
    gradient is 0.  Returns per-utterance losses (or their mean / sum over B); differentiable
    w.r.t. log_probs."""
    if input_lengths is None:
        return _CTCLoss.apply(log_probs, targets, blank, reduction)
    frames = _frame_counts("ctc_loss", input_lengths, log_probs.shape[0], log_probs.shape[1], 1)
    return _CTCLoss.apply(log_probs, targets, blank, reduction, frames)


def _flat_targets(targets):
    flat = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int32).reshape(-1) for t in targets])
                                if len(targets) else np.zeros(0, np.int32), dtype=np.int32)
    return flat, np.ascontiguousarray([len(t) for t in targets], dtype=np.int32)


def ctc_forced_align(log_probs, targets, blank=0, input_lengths=None):
    """CTC forced alignment of a batch, device-resident: the best path of target_b ∩ emissions_b (the reference's
    viterbiPath) for every utterance in one launch, nothing copied back.
    log_probs: float32 CUDA tensor [B, T, C] (any scores), read in place and left untouched; targets: B label
    sequences; input_lengths: per-utterance frame counts (<= T) or None.
    Returns (labels int32 [B, T], tokens int32 [B, T], scores float32 [B]) on log_probs.device: the label of every
    frame, the index of the frame's token in its target (-1 on blank frames), the path score.  Entries past an
    utterance's length are -1; an utterance no path fits has score -inf and rows of -1.  No autograd."""
    assert log_probs.is_cuda and log_probs.dtype == torch.float32 and log_probs.dim() == 3
    B, T, C = log_probs.shape
    if len(targets) != B:
        raise ValueError(f"ctc_forced_align: {len(targets)} target sequences for a batch of {B}")
    x = log_probs.detach().contiguous()
    frames = None if input_lengths is None else _frame_counts("ctc_forced_align", input_lengths, B, T, None)
    stream = _engine_stream(x.device)
    labels = torch.empty(B, T, dtype=torch.int32, device=x.device)
    tokens = torch.empty(B, T, dtype=torch.int32, device=x.device)
    scores = torch.empty(B, dtype=torch.float32, device=x.device)
    if _has_native("ctc_forced_align", "gtn_ctc_align_n", python_route=True):
        flat, lens = _flat_targets(targets)
        _call("gtn_ctc_align_n", x.data_ptr(), flat.ctypes.data, lens.ctypes.data, B, T, C, int(blank),
              _host_ptr(frames), labels.data_ptr(), tokens.data_ptr(), scores.data_ptr())
    else:
        ctcs = gtn.Batch.ctc_targets([list(t) for t in targets], blank, calc_grad=False)
        ems = gtn.Batch.linear(B, T, C, x, calc_grad=False, borrow=True)
        gtn.intersect(ctcs, ems).viterbi_align(labels, tokens, scores, frames)
    _engine_done(stream)
    return labels, tokens, scores


class _ASGLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emissions, transitions, start, targets, reduction, frames=None):
        assert emissions.is_cuda and emissions.dtype == torch.float32 and emissions.dim() == 3
        B, T, N = emissions.shape
        assert transitions.shape == (N, N) and start.shape == (N,)
        if len(targets) != B:
            raise ValueError(f"asg_loss: {len(targets)} target sequences for a batch of {B}")
        lib = _native()
        if not lib:
            raise RuntimeError("asg_loss needs gtn_amd/lib/libgtn_criteria.so (run __graft_entry__.build())")
        x = emissions.contiguous()
        # arc order of gtn::criteria::asgTransitions: N start arcs, then arc N + i*N + j = j -> i
        w = torch.cat([start.reshape(-1), transitions.reshape(-1)]).to(torch.float32).contiguous()
        stream = torch.cuda.current_stream(x.device)
        gtn.set_stream(stream.cuda_stream if stream.cuda_stream else None)
        if not stream.cuda_stream:
            stream.synchronize()
        flat, lens = _flat_targets(targets)
        out = torch.empty(B, dtype=torch.float32, device=x.device)
        gem = torch.empty(B, T, N, dtype=torch.float32, device=x.device) if emissions.requires_grad else None
        need_tr = transitions.requires_grad or start.requires_grad
        gtr = torch.empty(N + N * N, dtype=torch.float32, device=x.device) if need_tr else None
        ctx.ragged = frames is not None
        if frames is None:
            rc = lib.gtn_asg_loss_n(x.data_ptr(), flat.ctypes.data, lens.ctypes.data, B, T, N, w.data_ptr(),
                                    out.data_ptr(), gem.data_ptr() if gem is not None else None,
                                    gtr.data_ptr() if gtr is not None else None)
        else:
            if not hasattr(lib, "gtn_asg_loss_frames_n"):
                raise RuntimeError("asg_loss(input_lengths=...) needs gtn_asg_loss_frames_n in "
                                   "gtn_amd/lib/libgtn_criteria.so (run __graft_entry__.build())")
            rc = lib.gtn_asg_loss_frames_n(x.data_ptr(), flat.ctypes.data, lens.ctypes.data, B, T, N, w.data_ptr(),
                                           frames.ctypes.data, out.data_ptr(),
                                           gem.data_ptr() if gem is not None else None,
                                           gtr.data_ptr() if gtr is not None else None)
        if rc != 0:
            raise RuntimeError(lib.gtn_criteria_last_error().decode())
        if not stream.cuda_stream:
            gtn.synchronize()
        ctx.grads = (gem, gtr)
        ctx.shape = (B, T, N)
        ctx.reduction = reduction
        ctx.per_utterance = reduction == "none"
        return out.mean() if reduction == "mean" else (out.sum() if reduction == "sum" else out)

    @staticmethod
    def backward(ctx, grad_out):
        B, T, N = ctx.shape
        gem, gtr = ctx.grads
        if ctx.per_utterance:
            # the transition gradient was summed over the batch with unit seeds (as
            # criterion_test.cpp:289-305 accumulates it); per-utterance seeds must be uniform
            scale_em = grad_out.reshape(B, 1, 1)
            scale_tr = grad_out.reshape(-1)[0] if gtr is not None else None
            if gtr is not None and not bool((grad_out == grad_out.reshape(-1)[0]).all()):
                raise RuntimeError("asg_loss(reduction='none'): transition gradients need a uniform upstream "
                                   "gradient; use reduction='sum' or 'mean'")
        else:
            scale_em = (grad_out / B if ctx.reduction == "mean" else grad_out).reshape(1, 1, 1)
            scale_tr = scale_em.reshape(())
        g_em = gem * scale_em if gem is not None else None
        g_tr = g_st = None
        if gtr is not None:
            g_st = gtr[:N] * scale_tr
            g_tr = gtr[N:].reshape(N, N) * scale_tr
        return (g_em, g_tr, g_st, None, None) + ((None,) if ctx.ragged else ())


def asg_loss(emissions, transitions, targets, start=None, reduction="none", input_lengths=None):
    """The ASG criterion of examples/asg.cpp:30-68 / criterion_test.cpp:182-306 for a batch.
    emissions: float32 CUDA [B, T, N]; transitions: [N, N] with transitions[i, j] the score of
    label j followed by label i; start: [N] scores of the first label (zeros when omitted);
    targets: B label sequences.  Differentiable w.r.t. emissions, transitions and start; the
    full-connect term runs on the symbolic composition (nothing of size T*N*N is stored).
    input_lengths: a sequence or int tensor of B frame counts (1 .. T) for a padded batch, or None: utterance
    b's loss is that of emissions[b, :T_b], rows past T_b are never read and their gradient is 0.  With N <= 128
    the full-connect term of a padded batch is one launch (one workgroup per utterance walks its own frames);
    larger alphabets run one group of launches per distinct length.  An utterance with T_b < len(target_b) has
    no alignment: its loss is +inf and its gradient rows hold the full-connect posteriors alone."""
    if start is None:
        start = torch.zeros(emissions.shape[-1], dtype=torch.float32, device=emissions.device)
    if input_lengths is None:
        return _ASGLoss.apply(emissions, transitions, start, targets, reduction)
    frames = _frame_counts("asg_loss", input_lengths, emissions.shape[0], emissions.shape[1], 1)
    return _ASGLoss.apply(emissions, transitions, start, targets, reduction, frames)


def _asg_transitions_graph(N, w):
    """gtn::criteria::asgTransitions(N) over the device weights `w` ([N + N*N]: N start arcs, then arc N + i*N + j =
    j -> i)"""
    g = gtn.Graph(False)
    g.add_nodes(np.array([1] + [0] * N, np.uint8), np.array([0] + [1] * N, np.uint8))
    n = np.arange(N)
    src = np.concatenate([np.zeros(N, np.int32), np.tile(n + 1, N).astype(np.int32)])
    dst = np.concatenate([n + 1, np.repeat(n + 1, N)]).astype(np.int32)
    lab = np.concatenate([n, np.repeat(n, N)]).astype(np.int32)
    g.add_arcs(src, dst, lab, lab, np.zeros(N + N * N, np.float32))
    g.arc_sort()
    g.set_weights_device(w)
    return g


def asg_forced_align(emissions, transitions, targets, start=None, input_lengths=None):
    """ASG forced alignment of a batch, device-resident: the best path of emissions_b o (forceAlign(target_b) o
    transitions) (the reference's viterbiPath over examples/asg.cpp:50-68) for every utterance in one launch, nothing
    copied back.
    emissions: float32 CUDA tensor [B, T, N] (any scores), read in place and left untouched; transitions: [N, N] with
    transitions[i, j] the score of label j followed by label i; start: [N] scores of the first label (zeros when
    omitted); targets: B label sequences over 0 .. N-1; input_lengths: per-utterance frame counts (0 .. T) or None.
    Returns (labels int32 [B, T], tokens int32 [B, T], scores float32 [B]) on emissions.device: the label of every
    frame, the index of that label in its target (which of two equal neighbours a frame belongs to; never -1 inside
    a path), the path score.  Entries past an utterance's length are -1; an utterance with fewer frames than labels
    (or with no labels) has score -inf and rows of -1.  Of two exactly equal candidates the step to the next label
    wins, as in the reference.  No autograd.
    The launch takes N a multiple of 4 with 4 <= N <= 2048 and targets of at most 511 labels; any other shape raises
    the engine's error (token indices and frame counts do not exist on the path-graph route)."""
    assert emissions.is_cuda and emissions.dtype == torch.float32 and emissions.dim() == 3
    B, T, N = emissions.shape
    if start is None:
        start = torch.zeros(N, dtype=torch.float32, device=emissions.device)
    assert transitions.shape == (N, N) and start.shape == (N,)
    if len(targets) != B:
        raise ValueError(f"asg_forced_align: {len(targets)} target sequences for a batch of {B}")
    frames = None if input_lengths is None else _frame_counts("asg_forced_align", input_lengths, B, T, 0)
    x = emissions.detach().contiguous()
    w = _asg_weights(start, transitions)
    stream = _engine_stream(x.device)
    labels = torch.empty(B, T, dtype=torch.int32, device=x.device)
    tokens = torch.empty(B, T, dtype=torch.int32, device=x.device)
    scores = torch.empty(B, dtype=torch.float32, device=x.device)
    if _has_native("asg_forced_align", "gtn_asg_align_n"):
        flat, lens = _flat_targets(targets)
        _call("gtn_asg_align_n", x.data_ptr(), flat.ctypes.data, lens.ctypes.data, B, T, N, w.data_ptr(),
              _host_ptr(frames), labels.data_ptr(), tokens.data_ptr(), scores.data_ptr())
    else:
        trans = _asg_transitions_graph(N, w)
        ems = gtn.Batch.linear(B, T, N, x, calc_grad=False, borrow=True)
        fals = gtn.Batch.asg_force_align([list(t) for t in targets], trans, N)
        gtn.compose(ems, fals).viterbi_align(labels, tokens, scores, frames)
    _engine_done(stream)
    return labels, tokens, scores


def asg_decode(emissions, transitions, start=None, input_lengths=None, collapse=False):
    """ASG Viterbi decode of a batch, device-resident: the best path of emissions_b o transitions (the reference's
    viterbiPath over the full-connect product of examples/asg.cpp:36-47) for every utterance -- one sweep of the padded
    batch and one launch whatever the lengths, nothing copied back.
    emissions: float32 CUDA tensor [B, T, N] (any scores), read in place and left untouched, pad rows included (what
    they hold, NaN included, never changes a bit of any output); transitions: [N, N] with transitions[i, j] the score
    of label j followed by label i; start: [N] scores of the first label (zeros when omitted); input_lengths:
    per-utterance frame counts (0 .. T) or None.
    Returns (labels int32 [B, T], scores float32 [B]) on emissions.device -- the label of every frame, -1 from the
    utterance's length on, and the path score -- and with collapse=True also (collapsed int32 [B, T], lengths int32
    [B]): the labels with runs of equal consecutive frames merged, -1 from the length on.  An utterance without frames
    has rows of -1, score -inf and length 0.  Of exactly equal candidates the smallest label wins, as in the reference.
    Runs on the caller's stream; no autograd.
    The launch takes 7 <= N <= 1023; any other N goes through viterbi_path and one upload, where input_lengths raises
    the engine's error."""
    if emissions.dim() != 3 or emissions.dtype != torch.float32:
        raise ValueError("asg_decode: emissions must be a float32 tensor [B, T, N]")
    B, T, N = emissions.shape
    if tuple(transitions.shape) != (N, N):
        raise ValueError(f"asg_decode: transitions must be [{N}, {N}]")
    if start is not None and tuple(start.shape) != (N,):
        raise ValueError(f"asg_decode: start must be [{N}]")
    frames = None if input_lengths is None else _frame_counts("asg_decode", input_lengths, B, T, 0)
    if not emissions.is_cuda:
        raise RuntimeError("asg_decode: emissions must be a CUDA tensor (the decode runs on the device)")
    if start is None:
        start = torch.zeros(N, dtype=torch.float32, device=emissions.device)
    x = emissions.detach().contiguous()
    w = _asg_weights(start, transitions)
    stream = _engine_stream(x.device)
    labels = torch.empty(B, T, dtype=torch.int32, device=x.device)
    scores = torch.empty(B, dtype=torch.float32, device=x.device)
    collapsed = torch.empty(B, T, dtype=torch.int32, device=x.device) if collapse else None
    lengths = torch.empty(B, dtype=torch.int32, device=x.device) if collapse else None
    if _has_native("asg_decode", "gtn_asg_decode_n"):
        _call("gtn_asg_decode_n", x.data_ptr(), B, T, N, w.data_ptr(), _host_ptr(frames), labels.data_ptr(),
              scores.data_ptr(), _ptr(collapsed), _ptr(lengths))
    else:
        trans = _asg_transitions_graph(N, w)
        ems = gtn.Batch.linear(B, T, N, x, calc_grad=False, borrow=True)
        ems.viterbi_decode(trans, labels, scores, frames, collapsed, lengths, row_stride=T)
    _engine_done(stream)
    return (labels, scores, collapsed, lengths) if collapse else (labels, scores)


def ctc_decode(log_probs, blank=0, input_lengths=None, collapse=True):
    """CTC best-path (greedy) decode of a batch, device-resident: the reference's viterbiPath(emissions_b) for every
    utterance of a padded batch, then the CTC collapse (merge repeats, drop blanks) -- two launches whatever the
    lengths, nothing copied back.
    log_probs: float32 CUDA tensor [B, T, C] (any scores), read in place and left untouched; rows past an utterance's
    length are never read; blank: the label the collapse drops (negative: none, repeats are merged only);
    input_lengths: per-utterance frame counts (0 .. T) or None.
    Returns (labels int32 [B, T], scores float32 [B]) on log_probs.device -- the label of every frame, -1 from the
    utterance's length on, and the path score, the float32 sum of the frame maxima in frame order -- and with
    collapse=True also (tokens int32 [B, T], starts int32 [B, T], lengths int32 [B]): the collapsed labels, the first
    frame of each, both -1 from the length on.  Of exactly equal maxima the smallest label wins, as in the reference;
    NaN and -inf are never chosen, and a frame with nothing above -inf leaves the utterance without a path: rows of
    -1, score -inf, length 0.  So does an utterance without frames (linearGraph(0, C) has no accepting node).
    Runs on the caller's stream; no autograd."""
    if log_probs.dim() != 3 or log_probs.dtype != torch.float32:
        raise ValueError("ctc_decode: log_probs must be a float32 tensor [B, T, C]")
    B, T, N = log_probs.shape
    blank = int(blank)
    if blank >= N:
        raise ValueError(f"ctc_decode: blank must be below the {N} labels (negative: no blank)")
    frames = None if input_lengths is None else _frame_counts("ctc_decode", input_lengths, B, T, 0)
    if not log_probs.is_cuda:
        raise RuntimeError("ctc_decode: log_probs must be a CUDA tensor (the decode runs on the device)")
    x = log_probs.detach().contiguous()
    stream = _engine_stream(x.device)
    labels = torch.empty(B, T, dtype=torch.int32, device=x.device)
    scores = torch.empty(B, dtype=torch.float32, device=x.device)
    tokens = torch.empty(B, T, dtype=torch.int32, device=x.device) if collapse else None
    starts = torch.empty(B, T, dtype=torch.int32, device=x.device) if collapse else None
    lengths = torch.empty(B, dtype=torch.int32, device=x.device) if collapse else None
    _route(stream, x, _has_native("ctc_decode", "gtn_ctc_decode_n"), "gtn_ctc_decode_n",
           (blank, _host_ptr(frames), labels.data_ptr(), scores.data_ptr(), _ptr(tokens), _ptr(starts), _ptr(lengths)),
           "linear_decode", labels, scores, frames, blank, tokens, starts, lengths, row_stride=T)
    return (labels, scores, tokens, starts, lengths) if collapse else (labels, scores)


def ctc_sample(log_probs, blank=0, input_lengths=None, num_samples=4, temperature=1.0, seed=None, return_labels=False):
    """`num_samples` label sequences per utterance drawn from the CTC posterior, device-resident: the frames of a CTC
    alignment are independent, so one categorical draw per frame plus the CTC collapse is an exact sample of P(y | x)
    -- one stream over the emissions and one collapse, two launches whatever the lengths, nothing copied back.  What
    sampled minimum Bayes risk, scheduled sampling and calibration need where `ctc_beam_decode` gives the top of the
    distribution.
    log_probs: float32 CUDA tensor [B, T, C] (any scores: frame t takes label c with probability
    exp(x[b, t, c] / temperature) / Z[b, t]), read in place and left untouched; rows past an utterance's length are
    never read; blank: the label the collapse drops (negative: none, repeats are merged only); input_lengths:
    per-utterance frame counts (0 .. T) or None; num_samples 1 .. 1024; temperature finite and > 0; seed: 0 .. 2^64 - 1
    keys the Philox4x32-10 counters (t, b, k), so a seed repeats a run bit for bit -- None takes one 63-bit integer
    from torch's default CPU generator, so that `torch.manual_seed` repeats a run, without a device sync.
    Returns (tokens int32 [B, num_samples, T], lengths int32 [B, num_samples], logq float32 [B, num_samples]) on
    log_probs.device -- the layout of `ctc_beam_decode`, which `ctc_score`, `edit_distance` and `ctc_token_align` take
    as it is: the collapsed alignment, -1 from its length on, and the log-probability of the drawn ALIGNMENT,
    sum_t (x / temperature - log Z), float32 in frame order (the sequence's own log-probability is `ctc_score` minus
    the sum of log Z).  With return_labels a fourth tensor, int32 [B, num_samples, T], has the frame labels, -1 from
    the utterance's length on.  Only finite entries carry mass: -inf, +inf and NaN are never drawn, and a frame
    without a finite entry, or an utterance without frames, leaves every sample of that utterance at -1, length 0 and
    logq -inf.  Runs on the caller's stream; no autograd."""
    if log_probs.dim() != 3 or log_probs.dtype != torch.float32:
        raise ValueError("ctc_sample: log_probs must be a float32 tensor [B, T, C]")
    B, T, N = log_probs.shape
    blank, num_samples, temperature = int(blank), int(num_samples), float(temperature)
    if blank >= N:
        raise ValueError(f"ctc_sample: blank must be below the {N} labels (negative: no blank)")
    if not 1 <= num_samples <= 1024:
        raise ValueError("ctc_sample: num_samples outside 1 .. 1024")
    if not (math.isfinite(temperature) and temperature > 0.0):
        raise ValueError("ctc_sample: temperature must be finite and above 0")
    frames = None if input_lengths is None else _frame_counts("ctc_sample", input_lengths, B, T, 0)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())  # (a CPU tensor: no device sync)
    seed = int(seed)
    if not 0 <= seed < (1 << 64):
        raise ValueError("ctc_sample: seed must be in 0 .. 2^64 - 1")
    if not log_probs.is_cuda:
        raise RuntimeError("ctc_sample: log_probs must be a CUDA tensor (the sampler runs on the device)")
    x = log_probs.detach().contiguous()
    stream = _engine_stream(x.device)
    tokens = torch.empty(B, num_samples, T, dtype=torch.int32, device=x.device)
    lengths = torch.empty(B, num_samples, dtype=torch.int32, device=x.device)
    logq = torch.empty(B, num_samples, dtype=torch.float32, device=x.device)
    labels = torch.empty(B, num_samples, T, dtype=torch.int32, device=x.device) if return_labels else None
    _route(stream, x, _has_native("ctc_sample", "gtn_ctc_sample_n"), "gtn_ctc_sample_n",
           (blank, _host_ptr(frames), num_samples, seed, temperature, tokens.data_ptr(), lengths.data_ptr(),
            logq.data_ptr(), _ptr(labels)),
           "ctc_sample", tokens, lengths, logq, labels, frames, blank, num_samples, seed, temperature, row_stride=T)
    return (tokens, lengths, logq, labels) if return_labels else (tokens, lengths, logq)


def ctc_beam_decode(log_probs, blank=0, input_lengths=None, beam_size=16, cutoff_top_n=16, nbest=1, transitions=None,
                    start=None, lm_weight=1.0, insertion_bonus=0.0, return_am_scores=False, lm_graph=None):
    """CTC prefix beam search of a batch with N-best output, device-resident: the best label sequences, summed over
    their alignments, where `ctc_decode` gives the best alignment -- two launches whatever the lengths, nothing copied
    back.
    log_probs: float32 CUDA tensor [B, T, C] (any scores), read in place and left untouched; rows past an utterance's
    length are never read; blank: the blank label (0 .. C - 1); input_lengths: per-utterance frame counts (0 .. T) or
    None; beam_size: prefixes kept per frame (1 .. 64); cutoff_top_n: the best labels of a frame that may extend a
    prefix (1 .. 32; blank is always offered where its score is above -inf); nbest: hypotheses returned (1 ..
    beam_size).
    Returns (tokens int32 [B, nbest, T], lengths int32 [B, nbest], scores float32 [B, nbest]) on log_probs.device, best
    first: the labels of each hypothesis, -1 from its length on, and its log score summed over the alignments the beam
    kept (float32 log-add; unpruned it is -ctc_loss of that sequence).  Of exactly equal scores the order is: a prefix
    that stayed before one that grew, then the parent's rank, then the label; NaN and -inf are never chosen.  Slots
    without a hypothesis -- fewer than nbest prefixes, a frame with nothing above -inf, an utterance without frames --
    get -1, length 0 and score -inf.  Runs on the caller's stream; no autograd.
    transitions [C, C] (and start [C], zeros if None): the bigram tables `asg_loss` learns, fused into the ranking --
    transitions[i, j] scores label j followed by label i, start[c] label c as the first.  Every label of a prefix adds
    lm_weight * (its table entry) + insertion_bonus to the prefix's language model score L (float32, left to right);
    candidates rank by acoustic total + L, a -inf entry forbids its bigram or first label, the cutoff_top_n pruning
    stays acoustic and rows and columns of `blank` are never read.  Both tables are detached and may be non-contiguous.
    `scores` is then acoustic + L; with return_am_scores a fourth tensor, float32 [B, nbest], has the acoustic total
    alone (unpruned, `ctc_score` of those tokens), -inf in empty slots.  transitions=None is the search without a
    language model, whatever the other four say.
    lm_graph: a `gtn_amd.LmGraph` -- a language model held as a graph, a deterministic acceptor with back-off arcs -- in
    the tables' place; giving both raises ValueError.  A prefix then also carries its state in the graph, and its labels
    add lm_weight * (the weight of the walk of (state, label), failure-arc semantics: `LmGraph.walk`) +
    insertion_bonus; a label the walk forbids is dropped.  lm_weight, insertion_bonus and return_am_scores mean what
    they mean with the tables.  The graph is a snapshot taken when the LmGraph was made: no gradient reaches it."""
    if lm_graph is not None:
        if transitions is not None or start is not None:
            raise ValueError("ctc_beam_decode: give either transitions / start or lm_graph, not both")
        if not isinstance(lm_graph, gtn.LmGraph):
            raise ValueError("ctc_beam_decode: lm_graph must be a gtn_amd.LmGraph")
        lm_weight, insertion_bonus = float(lm_weight), float(insertion_bonus)
        if not (math.isfinite(lm_weight) and math.isfinite(insertion_bonus)):
            raise ValueError("ctc_beam_decode: lm_weight and insertion_bonus must be finite")
    if log_probs.dim() != 3 or log_probs.dtype != torch.float32:
        raise ValueError("ctc_beam_decode: log_probs must be a float32 tensor [B, T, C]")
    B, T, N = log_probs.shape
    blank, beam_size, cutoff_top_n, nbest = int(blank), int(beam_size), int(cutoff_top_n), int(nbest)
    if not 0 <= blank < N:
        raise ValueError(f"ctc_beam_decode: blank must be one of the {N} labels")
    if not 1 <= beam_size <= 64:
        raise ValueError("ctc_beam_decode: beam_size outside 1 .. 64")
    if not 1 <= cutoff_top_n <= 32:
        raise ValueError("ctc_beam_decode: cutoff_top_n outside 1 .. 32")
    if not 1 <= nbest <= beam_size:
        raise ValueError("ctc_beam_decode: nbest outside 1 .. beam_size")
    frames = None if input_lengths is None else _frame_counts("ctc_beam_decode", input_lengths, B, T, 0)
    if transitions is not None:
        if transitions.dim() != 2 or tuple(transitions.shape) != (N, N):
            raise ValueError(f"ctc_beam_decode: transitions must be a tensor [{N}, {N}]")
        if start is not None and tuple(start.shape) != (N,):
            raise ValueError(f"ctc_beam_decode: start must be a tensor [{N}]")
        lm_weight, insertion_bonus = float(lm_weight), float(insertion_bonus)
        if not (math.isfinite(lm_weight) and math.isfinite(insertion_bonus)):
            raise ValueError("ctc_beam_decode: lm_weight and insertion_bonus must be finite")
    if not log_probs.is_cuda:
        raise RuntimeError("ctc_beam_decode: log_probs must be a CUDA tensor (the search runs on the device)")
    x = log_probs.detach().contiguous()
    table = None
    if transitions is not None:
        # (written on the caller's stream BEFORE the engine is pointed at it: on the null stream _engine_stream waits
        #  once for what is queued so far, and the engine's own stream is ordered with nothing that comes after)
        tr = transitions.detach().to(x.device)
        st = torch.zeros(N, dtype=torch.float32, device=x.device) if start is None else start.detach().to(x.device)
        table = _asg_weights(st, tr)
    stream = _engine_stream(x.device)
    tokens = torch.empty(B, nbest, T, dtype=torch.int32, device=x.device)
    lengths = torch.empty(B, nbest, dtype=torch.int32, device=x.device)
    scores = torch.empty(B, nbest, dtype=torch.float32, device=x.device)
    if lm_graph is not None:
        am = torch.empty(B, nbest, dtype=torch.float32, device=x.device) if return_am_scores else None
        _route(stream, x, _has_native("ctc_beam_decode", "gtn_ctc_beam_decode_graph_n"), "gtn_ctc_beam_decode_graph_n",
               (blank, _host_ptr(frames), beam_size, cutoff_top_n, nbest, lm_graph._h, lm_weight, insertion_bonus,
                tokens.data_ptr(), lengths.data_ptr(), scores.data_ptr(), _ptr(am)),
               "ctc_beam_decode", tokens, lengths, scores, frames, blank, beam_size, cutoff_top_n, nbest, row_stride=T,
               lm=lm_graph, lm_weight=lm_weight, insertion_bonus=insertion_bonus, am_scores_out=am)
        return (tokens, lengths, scores, am) if return_am_scores else (tokens, lengths, scores)
    if table is not None:
        am = torch.empty(B, nbest, dtype=torch.float32, device=x.device) if return_am_scores else None
        _route(stream, x, _has_native("ctc_beam_decode", "gtn_ctc_beam_decode_lm_n"), "gtn_ctc_beam_decode_lm_n",
               (blank, _host_ptr(frames), beam_size, cutoff_top_n, nbest, table.data_ptr(), lm_weight, insertion_bonus,
                tokens.data_ptr(), lengths.data_ptr(), scores.data_ptr(), _ptr(am)),
               "ctc_beam_decode", tokens, lengths, scores, frames, blank, beam_size, cutoff_top_n, nbest, row_stride=T,
               lm=table, lm_weight=lm_weight, insertion_bonus=insertion_bonus, am_scores_out=am)
        return (tokens, lengths, scores, am) if return_am_scores else (tokens, lengths, scores)
    _route(stream, x, _has_native("ctc_beam_decode", "gtn_ctc_beam_decode_n"), "gtn_ctc_beam_decode_n",
           (blank, _host_ptr(frames), beam_size, cutoff_top_n, nbest, tokens.data_ptr(), lengths.data_ptr(),
            scores.data_ptr()),
           "ctc_beam_decode", tokens, lengths, scores, frames, blank, beam_size, cutoff_top_n, nbest, row_stride=T)
    return tokens, lengths, scores


def asg_beam_decode(emissions, transitions, start=None, input_lengths=None, beam_size=16, cutoff_top_n=16, nbest=1,
                    lm_graph=None, lm_weight=1.0, insertion_bonus=0.0, return_am_scores=False):
    """ASG prefix beam search of a batch with N-best output, device-resident: the best label sequences without equal
    neighbours -- the sequences `asg_decode(collapse=True)` can emit -- each summed over all of its alignments under
    emissions o transitions, where `asg_decode` gives the best alignment.  Two launches whatever the lengths, nothing
    copied back.
    emissions: float32 CUDA tensor [B, T, N] (any scores), read in place and left untouched; rows past an utterance's
    length are never read; transitions: [N, N] with transitions[i, j] the score of label j followed by label i; start:
    [N] scores of the first label (zeros when omitted) -- both detached, and a -inf entry forbids its bigram or first
    label; input_lengths: per-utterance frame counts (0 .. T) or None; beam_size: prefixes kept per frame (1 .. 64);
    cutoff_top_n: the best labels of a frame that a prefix may stay in or grow by (1 .. 32); nbest: hypotheses returned
    (1 .. beam_size).
    Returns (tokens int32 [B, nbest, T], lengths int32 [B, nbest], scores float32 [B, nbest]) on emissions.device, best
    first: the labels of each hypothesis, -1 from its length on, and its log score summed over the alignments the beam
    kept (float32 log-add; unpruned it is `asg_score` of that sequence).  Of exactly equal scores the order is: a prefix
    that stayed before one that grew, then the parent's rank, then the label; NaN and -inf are never chosen.  Slots
    without a hypothesis -- fewer than nbest prefixes, a frame with nothing above -inf, an utterance without frames --
    get -1, length 0 and score -inf.  The outputs feed `asg_score` and `edit_distance` as they are.  Runs on the
    caller's stream and does not wait; no autograd.
    lm_graph: a `gtn_amd.LmGraph` -- a language model held as a graph: a lexicon, a grammar, an n-gram model with
    back-off arcs -- fused into the ranking; `transitions` and `start` stay the criterion's own.  A prefix then also
    carries its state in the graph, and each of its labels adds lm_weight * (the weight of the walk of (state, label),
    failure-arc semantics: `LmGraph.walk`) + insertion_bonus to its LM score L; a label the walk forbids is dropped.
    Hypotheses rank by acoustic score + L, which is what `scores` then holds; with return_am_scores a fourth tensor,
    float32 [B, nbest], has the acoustic score alone (unpruned, `asg_score` of those tokens), -inf in empty slots.  The
    graph is a snapshot taken when the LmGraph was made: no gradient reaches it.  ValueError: an lm_graph that is no
    LmGraph, a weight or bonus that is not finite, and lm_weight, insertion_bonus or return_am_scores without
    lm_graph."""
    if lm_graph is None:
        if lm_weight != 1.0 or insertion_bonus != 0.0 or return_am_scores:
            raise ValueError("asg_beam_decode: lm_weight, insertion_bonus and return_am_scores need lm_graph")
    else:
        if not isinstance(lm_graph, gtn.LmGraph):
            raise ValueError("asg_beam_decode: lm_graph must be a gtn_amd.LmGraph")
        lm_weight, insertion_bonus = float(lm_weight), float(insertion_bonus)
        if not (math.isfinite(lm_weight) and math.isfinite(insertion_bonus)):
            raise ValueError("asg_beam_decode: lm_weight and insertion_bonus must be finite")
    if emissions.dim() != 3 or emissions.dtype != torch.float32:
        raise ValueError("asg_beam_decode: emissions must be a float32 tensor [B, T, N]")
    B, T, N = emissions.shape
    beam_size, cutoff_top_n, nbest = int(beam_size), int(cutoff_top_n), int(nbest)
    if transitions.dim() != 2 or tuple(transitions.shape) != (N, N):
        raise ValueError(f"asg_beam_decode: transitions must be [{N}, {N}]")
    if start is not None and tuple(start.shape) != (N,):
        raise ValueError(f"asg_beam_decode: start must be [{N}]")
    if not 1 <= beam_size <= 64:
        raise ValueError("asg_beam_decode: beam_size outside 1 .. 64")
    if not 1 <= cutoff_top_n <= 32:
        raise ValueError("asg_beam_decode: cutoff_top_n outside 1 .. 32")
    if not 1 <= nbest <= beam_size:
        raise ValueError("asg_beam_decode: nbest outside 1 .. beam_size")
    frames = None if input_lengths is None else _frame_counts("asg_beam_decode", input_lengths, B, T, 0)
    if not emissions.is_cuda:
        raise RuntimeError("asg_beam_decode: emissions must be a CUDA tensor (the search runs on the device)")
    x = emissions.detach().contiguous()
    # (written on the caller's stream BEFORE the engine is pointed at it: on the null stream _engine_stream waits once
    #  for what is queued so far, and the engine's own stream is ordered with nothing that comes after)
    tr = transitions.detach().to(x.device)
    st = torch.zeros(N, dtype=torch.float32, device=x.device) if start is None else start.detach().to(x.device)
    table = _asg_weights(st, tr)
    stream = _engine_stream(x.device)
    tokens = torch.empty(B, nbest, T, dtype=torch.int32, device=x.device)
    lengths = torch.empty(B, nbest, dtype=torch.int32, device=x.device)
    scores = torch.empty(B, nbest, dtype=torch.float32, device=x.device)
    if lm_graph is not None:
        am = torch.empty(B, nbest, dtype=torch.float32, device=x.device) if return_am_scores else None
        _route(stream, x, _has_native("asg_beam_decode", "gtn_asg_beam_decode_graph_n"), "gtn_asg_beam_decode_graph_n",
               (table.data_ptr(), _host_ptr(frames), beam_size, cutoff_top_n, nbest, lm_graph._h, lm_weight,
                insertion_bonus, tokens.data_ptr(), lengths.data_ptr(), scores.data_ptr(), _ptr(am)),
               "asg_beam_decode", tokens, lengths, scores, frames, table, beam_size, cutoff_top_n, nbest, row_stride=T,
               lm=lm_graph, lm_weight=lm_weight, insertion_bonus=insertion_bonus, am_scores_out=am)
        return (tokens, lengths, scores, am) if return_am_scores else (tokens, lengths, scores)
    _route(stream, x, _has_native("asg_beam_decode", "gtn_asg_beam_decode_n"), "gtn_asg_beam_decode_n",
           (table.data_ptr(), _host_ptr(frames), beam_size, cutoff_top_n, nbest, tokens.data_ptr(), lengths.data_ptr(),
            scores.data_ptr()),
           "asg_beam_decode", tokens, lengths, scores, frames, table, beam_size, cutoff_top_n, nbest, row_stride=T)
    return tokens, lengths, scores


def asg_sample(emissions, transitions, start=None, input_lengths=None, num_samples=4, temperature=1.0, seed=None,
               return_labels=False, return_logz=False):
    """`num_samples` label sequences per utterance drawn from the posterior of the ASG model emissions o transitions,
    device-resident.  ASG frames are not independent, so a draw per frame would be wrong: the call runs a log-semiring
    forward sweep that keeps the alpha planes, then samples backward from them (forward filtering, backward sampling),
    which is an exact sample -- alignment y comes with probability exp(s(y) / temperature - logZ), s(y) = start[y_0] +
    x[0, y_0] + sum_t (transitions[y_t, y_{t-1}] + x[t, y_t]) -- then merges equal neighbours.  What sampled minimum
    Bayes risk, scheduled sampling and calibration need where `asg_beam_decode` gives the top of the distribution.
    emissions: float32 CUDA tensor [B, T, N] (any scores), read in place and left untouched; rows past an utterance's
    length are never read; transitions: [N, N] with transitions[i, j] the score of label j followed by label i; start:
    [N] scores of the first label (zeros when omitted) -- both detached; 1 <= N <= 1024; input_lengths: per-utterance
    frame counts (0 .. T) or None; num_samples 1 .. 1024; temperature finite and > 0; seed: 0 .. 2^64 - 1 keys the
    Philox4x32-10 counters (t, b, k), so a seed repeats a run bit for bit -- None takes one 63-bit integer from torch's
    default CPU generator, so that `torch.manual_seed` repeats a run, without a device sync.
    Returns (tokens int32 [B, num_samples, T], lengths int32 [B, num_samples], logq float32 [B, num_samples]) on
    emissions.device -- the layout of `asg_beam_decode`, which `asg_score`, `edit_distance` and `asg_token_align` take
    as it is: the merged alignment, -1 from its length on, and the log-probability of the drawn ALIGNMENT, s(y) /
    temperature - logZ, added in float32 in draw order (the sequence's own log-probability is `asg_score` minus logZ).
    With return_labels a further tensor, int32 [B, num_samples, T], has the frame labels, -1 from the utterance's
    length on; with return_logz a last one, float32 [B], has logZ -- at temperature 1 the full-connect term of
    `asg_loss`.  Only finite entries carry mass: a -inf, +inf or NaN emission, transition or start score is never on a
    drawn path, and an utterance without an alignment of finite score, or without frames, leaves every sample of it at
    -1, length 0 and logq -inf, and logZ at -inf.  Runs on the caller's stream; no autograd."""
    if emissions.dim() != 3 or emissions.dtype != torch.float32:
        raise ValueError("asg_sample: emissions must be a float32 tensor [B, T, N]")
    B, T, N = emissions.shape
    num_samples, temperature = int(num_samples), float(temperature)
    if transitions.dim() != 2 or tuple(transitions.shape) != (N, N):
        raise ValueError(f"asg_sample: transitions must be [{N}, {N}]")
    if start is not None and tuple(start.shape) != (N,):
        raise ValueError(f"asg_sample: start must be [{N}]")
    if not 1 <= N <= 1024:
        raise ValueError("asg_sample: the number of labels is outside 1 .. 1024")
    if not 1 <= num_samples <= 1024:
        raise ValueError("asg_sample: num_samples outside 1 .. 1024")
    if not (math.isfinite(temperature) and temperature > 0.0):
        raise ValueError("asg_sample: temperature must be finite and above 0")
    frames = None if input_lengths is None else _frame_counts("asg_sample", input_lengths, B, T, 0)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())  # (a CPU tensor: no device sync)
    seed = int(seed)
    if not 0 <= seed < (1 << 64):
        raise ValueError("asg_sample: seed must be in 0 .. 2^64 - 1")
    if not emissions.is_cuda:
        raise RuntimeError("asg_sample: emissions must be a CUDA tensor (the sampler runs on the device)")
    x = emissions.detach().contiguous()
    # (written on the caller's stream BEFORE the engine is pointed at it, as in asg_beam_decode)
    tr = transitions.detach().to(x.device)
    st = torch.zeros(N, dtype=torch.float32, device=x.device) if start is None else start.detach().to(x.device)
    table = _asg_weights(st, tr)
    stream = _engine_stream(x.device)
    tokens = torch.empty(B, num_samples, T, dtype=torch.int32, device=x.device)
    lengths = torch.empty(B, num_samples, dtype=torch.int32, device=x.device)
    logq = torch.empty(B, num_samples, dtype=torch.float32, device=x.device)
    labels = torch.empty(B, num_samples, T, dtype=torch.int32, device=x.device) if return_labels else None
    logz = torch.empty(B, dtype=torch.float32, device=x.device) if return_logz else None
    _route(stream, x, _has_native("asg_sample", "gtn_asg_sample_n"), "gtn_asg_sample_n",
           (table.data_ptr(), _host_ptr(frames), num_samples, seed, temperature, tokens.data_ptr(), lengths.data_ptr(),
            logq.data_ptr(), _ptr(labels), _ptr(logz)),
           "asg_sample", tokens, lengths, table, logq, labels, logz, frames, num_samples, seed, temperature,
           row_stride=T)
    out = (tokens, lengths, logq)
    if return_labels:
        out += (labels,)
    if return_logz:
        out += (logz,)
    return out


def edit_distance(hyp, hyp_lengths, ref, ref_lengths, return_ops=False):
    """Levenshtein distance of hypotheses against references, device-resident: one launch (with `return_ops`, one per
    slice of pairs), nothing copied back -- `edit_distance(*ctc_beam_decode(...)[:2], ref, ref_lengths)` has no host
    round trip, and a `min` over the nbest axis of the result is the oracle error count.
    hyp: int32 CUDA tensor [B, N, L] (the `ctc_beam_decode` form) or [B, L] (the `ctc_decode` form); hyp_lengths: int32
    or int64 CUDA tensor [B, N] / [B]; ref: int32 CUDA tensor [B, U]; ref_lengths: int32 or int64 CUDA tensor [B].
    Lengths are read on the device and clamped to 0 .. L / 0 .. U there (a negative one counts as 0); elements at or
    past a length are never read, so a slot without a hypothesis (length 0, tokens -1) scores the reference's length.
    Tokens are compared with == only: any int32 is a token.  L <= 65536, U <= 4096.
    Returns dist, int32 [B, N] (or [B] for a [B, L] hyp), on hyp.device: unit costs for substitution, insertion and
    deletion.  With return_ops also ops, int32 [B, N, 3] (or [B, 3]) = (substitutions, deletions, insertions) of the
    walk back from the last cell that takes the diagonal where it attains the distance, else up (a deletion: a
    reference token without counterpart), else left (an insertion); they sum to dist.  Runs on the caller's stream;
    no autograd."""
    if not (torch.is_tensor(hyp) and hyp.dtype == torch.int32 and hyp.dim() in (2, 3)):
        raise ValueError("edit_distance: hyp must be an int32 tensor [B, N, L] or [B, L]")
    flat = hyp.dim() == 2
    B, N, L = (hyp.shape[0], 1, hyp.shape[1]) if flat else hyp.shape
    if not (torch.is_tensor(ref) and ref.dtype == torch.int32 and ref.dim() == 2 and ref.shape[0] == B):
        raise ValueError(f"edit_distance: ref must be an int32 tensor [B, U] for a batch of {B}")
    U = ref.shape[1]
    for t, shape, what in ((hyp_lengths, (B,) if flat else (B, N), "hyp_lengths"), (ref_lengths, (B,), "ref_lengths")):
        if not (torch.is_tensor(t) and t.dtype in (torch.int32, torch.int64) and tuple(t.shape) == tuple(shape)):
            raise ValueError(f"edit_distance: {what} must be an int32 or int64 tensor {list(shape)}")
    if L > 65536 or U > 4096:
        raise ValueError("edit_distance: rows wider than the kernel takes (L <= 65536, U <= 4096)")
    for t, what in ((hyp, "hyp"), (hyp_lengths, "hyp_lengths"), (ref, "ref"), (ref_lengths, "ref_lengths")):
        if not t.is_cuda:
            raise RuntimeError(f"edit_distance: {what} must be a CUDA tensor (the distances are computed on the device)")
        if t.device != hyp.device:
            raise ValueError("edit_distance: all tensors must be on one device")
    h, r = hyp.detach().contiguous(), ref.detach().contiguous()
    if B * N and h.numel() == 0:
        h = h.new_empty(1)  # (rows without an element are never read, but an empty tensor has no address)
    if B * N and r.numel() == 0:
        r = r.new_empty(1)
    hl = hyp_lengths.detach().to(torch.int32).contiguous()  # (int64 lengths are converted on the device)
    rl = ref_lengths.detach().to(torch.int32).contiguous()
    stream = _engine_stream(h.device)
    dist = torch.empty(B, N, dtype=torch.int32, device=h.device)
    ops = torch.empty(B, N, 3, dtype=torch.int32, device=h.device) if return_ops else None
    if B * N == 0:
        pass  # (no pair: nothing to launch, and an empty tensor has no address to hand over)
    elif _has_native("edit_distance", "gtn_edit_distance_n", python_route=True):
        _call("gtn_edit_distance_n", h.data_ptr(), hl.data_ptr(), r.data_ptr(), rl.data_ptr(), B, N, L, U,
              dist.data_ptr(), _ptr(ops))
    else:
        gtn.edit_distance(h.data_ptr(), hl.data_ptr(), r.data_ptr(), rl.data_ptr(), dist.data_ptr(), _ptr(ops),
                          B=B, N=N, L=L, U=U, hyp_stride=L, ref_stride=U)
    _engine_done(stream)
    if flat:
        dist = dist.reshape(B)
        ops = ops.reshape(B, 3) if return_ops else None
    return (dist, ops) if return_ops else dist


class _CTCScore(torch.autograd.Function):
    """forward: one launch that stores nothing but the scores; backward: the one gradient call with grad_out as the
    weights.  The node keeps tensors only: the backward recomputes what it needs."""

    @staticmethod
    def forward(ctx, log_probs, tokens, lengths, blank, frames, max_length):
        B, N, L = tokens.shape
        x = log_probs.detach().contiguous()
        stream = _engine_stream(x.device)
        scores = torch.empty(B, N, dtype=torch.float32, device=x.device)
        if B * N == 0:
            _engine_done(stream)  # (no pair: nothing to launch, and an empty tensor has no address to hand over)
        else:
            _route(stream, x, _has_native("ctc_score", "gtn_ctc_score_n"), "gtn_ctc_score_n",
                   (blank, _host_ptr(frames), tokens.data_ptr(), lengths.data_ptr(), N, L, max_length,
                    scores.data_ptr()),
                   "ctc_score", tokens.data_ptr(), lengths.data_ptr(), scores.data_ptr(), frames, blank, max_length,
                   N=N, L=L, row_stride=L)
        ctx.save_for_backward(x, tokens, lengths)
        ctx.args = (blank, frames, max_length)
        return scores

    @staticmethod
    def backward(ctx, grad_out):
        x, tokens, lengths = ctx.saved_tensors
        blank, frames, max_length = ctx.args
        B, T, C_ = x.shape
        N, L = tokens.shape[1], tokens.shape[2]
        if B * N == 0 or x.numel() == 0:
            return torch.zeros_like(x), None, None, None, None, None
        w = grad_out.detach().to(torch.float32).contiguous()
        stream = _engine_stream(x.device)
        grad = torch.empty(B, T, C_, dtype=torch.float32, device=x.device)
        _route(stream, x, _native(), "gtn_ctc_score_grad_n",
               (blank, _host_ptr(frames), tokens.data_ptr(), lengths.data_ptr(), N, L, max_length, w.data_ptr(),
                grad.data_ptr()),
               "ctc_score_grad", tokens.data_ptr(), lengths.data_ptr(), w.data_ptr(), grad.data_ptr(), frames, blank,
               max_length, N=N, L=L, row_stride=L)
        return grad, None, None, None, None, None


def ctc_score(log_probs, tokens, lengths, blank=0, input_lengths=None, max_length=None):
    """The exact log score of device-resident hypotheses under the emissions, differentiable: score[b, k] =
    forwardScore(ctcGraph(tokens[b, k, :len], blank) o log_probs[b, :T_b]), the log-sum over all alignments of the summed
    emissions, for all B * N hypotheses in one launch against the B shared slabs -- no download of the tokens, no wait, no
    repeated emissions.  No normaliser is subtracted: `ctc_loss(x, [y]) == forwardScore(x) - ctc_score(x, y)`, and an
    unpruned `ctc_beam_decode` gives the same number as its score.  It is the middle term of N-best objectives
    (`ctc_beam_decode` -> `ctc_score` -> `edit_distance` -> softmax-weighted risk).
    log_probs: float32 CUDA tensor [B, T, C] (any scores), read in place; tokens: int32 CUDA tensor [B, N, L] (the
    `ctc_beam_decode` form) or [B, L]; lengths: int32 or int64 CUDA tensor [B, N] / [B], read on the device and clamped to
    0 .. L there (a negative one counts as 0) -- elements at or past a length are never read; blank: 0 .. C - 1 (a token
    equal to blank is a label like any other); input_lengths: per-utterance frame counts (0 .. T) or None -- rows past
    T_b are never read and their gradient is exactly 0; max_length (1 .. 4096, default min(L, T, 4096)): the caller's
    bound on the hypotheses' lengths, which sizes the kernel's LDS and the backward's scratch.
    Returns float32 [B, N] (or [B]).  A score is -inf, with zero gradient and never NaN, when no alignment fits (length
    + repeats > T_b), every path crosses a -inf emission, the length is above max_length, a token inside the length lies
    outside 0 .. C - 1, or T_b == 0.  A beam slot WITHOUT a hypothesis (length 0, tokens -1) scores as the empty
    sequence, all blanks, which is a finite number: mask such slots with the -inf of the beam's own scores
    (`torch.where(beam_scores == -inf, beam_scores, score)`).
    The backward is one call that returns sum_k grad_out[b, k] * d score[b, k] / d log_probs; it recomputes what it
    needs (the node keeps tensors only), skips pairs whose score is -inf or whose incoming gradient is exactly 0, and
    sums in a fixed order without atomics, so it has the same bits run to run.  Without requires_grad it never launches.
    Runs on the caller's stream."""
    blank = int(blank)
    B, _, _, _, _, flat, tok, ln, frames, max_length = _hypothesis_args(
        "ctc_score", "scores", log_probs, "log_probs", tokens, lengths, blank, input_lengths, max_length)
    out = _CTCScore.apply(log_probs, tok, ln, blank, frames, max_length)
    return out.reshape(B) if flat else out


class _CTCLatticeScore(torch.autograd.Function):
    """forward: one launch that stores nothing but the scores; backward: the one gradient call with grad_out as the
    weights, asked for the arcs' gradient as well when the arc weights require one.  The node keeps tensors only."""

    @staticmethod
    def forward(ctx, log_probs, arc_weights, arcs, num_arcs, num_nodes, blank, frames, max_states):
        B, A = arcs.shape[:2]
        x = log_probs.detach().contiguous()
        w = None if arc_weights is None else arc_weights.detach().to(torch.float32).contiguous()
        stream = _engine_stream(x.device)
        scores = torch.empty(B, dtype=torch.float32, device=x.device)
        if B == 0:
            _engine_done(stream)  # (no utterance: nothing to launch, and an empty tensor has no address to hand over)
        else:
            _route(stream, x, _has_native("ctc_lattice_score", "gtn_ctc_lattice_score_n"), "gtn_ctc_lattice_score_n",
                   (blank, _host_ptr(frames), arcs.data_ptr(), num_arcs.data_ptr(), num_nodes.data_ptr(), _ptr(w), A,
                    max_states, scores.data_ptr()),
                   "ctc_lattice_score", arcs.data_ptr(), num_arcs.data_ptr(), num_nodes.data_ptr(), scores.data_ptr(),
                   _ptr(w), frames, blank, max_states, A=A, row_stride=3 * A)
        ctx.save_for_backward(x, arcs, num_arcs, num_nodes, *(() if w is None else (w,)))
        ctx.args = (blank, frames, max_states, None if arc_weights is None else arc_weights.dtype)
        return scores

    @staticmethod
    def backward(ctx, grad_out):
        x, arcs, num_arcs, num_nodes, *rest = ctx.saved_tensors
        w = rest[0] if rest else None
        blank, frames, max_states, w_dtype = ctx.args
        B, T, C_ = x.shape
        A = arcs.shape[1]
        want_w = w is not None and ctx.needs_input_grad[1]
        none = (None,) * 6
        if B == 0 or x.numel() == 0:
            return (torch.zeros_like(x), torch.zeros(B, A, dtype=w_dtype, device=x.device) if want_w else None) + none
        g = grad_out.detach().to(torch.float32).contiguous()
        stream = _engine_stream(x.device)
        grad = torch.empty(B, T, C_, dtype=torch.float32, device=x.device)
        garc = torch.empty(B, A, dtype=torch.float32, device=x.device) if want_w else None
        _route(stream, x, _native(), "gtn_ctc_lattice_score_grad_n",
               (blank, _host_ptr(frames), arcs.data_ptr(), num_arcs.data_ptr(), num_nodes.data_ptr(), _ptr(w), A,
                max_states, g.data_ptr(), grad.data_ptr(), _ptr(garc)),
               "ctc_lattice_score_grad", arcs.data_ptr(), num_arcs.data_ptr(), num_nodes.data_ptr(), g.data_ptr(),
               grad.data_ptr(), _ptr(garc), _ptr(w), frames, blank, max_states, A=A, row_stride=3 * A)
        return (grad, garc.to(w_dtype) if want_w else None) + none


def _lattice_args(who, log_probs, arcs, num_arcs, num_nodes, arc_weights, blank, input_lengths, max_states):
    """what `ctc_lattice_score` and `ctc_lattice_align` check of their arguments alike.  Returns (A, arcs contiguous,
    num_arcs and num_nodes as int32, blank, frames or None, max_states)"""
    x = log_probs
    if not (torch.is_tensor(x) and x.dim() == 3 and x.dtype == torch.float32):
        raise ValueError(f"{who}: log_probs must be a float32 tensor [B, T, C]")
    B, T, C_ = x.shape
    if not (torch.is_tensor(arcs) and arcs.dtype == torch.int32 and arcs.dim() == 3 and arcs.shape[0] == B
            and arcs.shape[2] == 3):
        raise ValueError(f"{who}: arcs must be an int32 tensor [B, A, 3] for a batch of {B}")
    A = arcs.shape[1]
    for t, name in ((num_arcs, "num_arcs"), (num_nodes, "num_nodes")):
        if not (torch.is_tensor(t) and t.dtype in (torch.int32, torch.int64) and tuple(t.shape) == (B,)):
            raise ValueError(f"{who}: {name} must be an int32 or int64 tensor [{B}]")
    if arc_weights is not None and not (torch.is_tensor(arc_weights) and arc_weights.is_floating_point()
                                        and tuple(arc_weights.shape) == (B, A)):
        raise ValueError(f"{who}: arc_weights must be a floating-point tensor [{B}, {A}]")
    blank = int(blank)
    if not 0 <= blank < C_:
        raise ValueError(f"{who}: blank must be one of the {C_} labels")
    max_states = max(1, min(2 * A + 1, 4096)) if max_states is None else int(max_states)
    if not 1 <= max_states <= 4096:
        raise ValueError(f"{who}: max_states outside 1 .. 4096")
    frames = None if input_lengths is None else _frame_counts(who, input_lengths, B, T, 0)
    for t, what in ((x, "log_probs"), (arcs, "arcs"), (num_arcs, "num_arcs"), (num_nodes, "num_nodes"),
                    (arc_weights, "arc_weights")):
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"{who}: {what} must be a CUDA tensor (the scores are computed on the device)")
        if t.device != x.device:
            raise ValueError(f"{who}: all tensors must be on one device")
    arcs_c = arcs.detach().contiguous()
    na = num_arcs.detach().to(torch.int32).contiguous()  # (int64 counts are converted on the device)
    nn_ = num_nodes.detach().to(torch.int32).contiguous()
    return A, arcs_c, na, nn_, blank, frames, max_states


def ctc_lattice_score(log_probs, arcs, num_arcs, num_nodes, arc_weights=None, blank=0, input_lengths=None,
                      max_states=None):
    """The exact CTC log score of one acyclic token lattice per utterance, differentiable: score[b] = log sum over the
    lattice's paths p of exp(w(p) + ctc_score(log_probs[b, :T_b], labels(p))) -- every word-piece decomposition,
    pronunciation or optional token the lattice holds and every alignment of each, marginalised in one launch; the
    lattices are read where they lie on the device.  No normaliser is subtracted (`ctc_lattice_loss` does that).
    log_probs: float32 CUDA tensor [B, T, C] (any scores), read in place; arcs: int32 CUDA tensor [B, A, 3] of (src, dst,
    label) rows with 0 <= src < dst < num_nodes[b], sorted by dst within an utterance (`gtn_amd.pack_lattices` gives
    this form); num_arcs, num_nodes: int32 or int64 CUDA tensors [B] -- node 0 starts, node num_nodes - 1 accepts, arcs
    at or past num_arcs[b] are never read; arc_weights: float32 CUDA tensor [B, A] or None (zeros), added once per use
    of an arc, -inf forbids it; blank: 0 .. C - 1 (a label equal to blank is a label like any other); input_lengths:
    per-utterance frame counts (0 .. T) or None -- rows past T_b are never read and their gradient is exactly 0;
    max_states (1 .. 4096, default min(2 A + 1, 4096)): the caller's bound on nodes + arcs, which sizes the kernel's
    LDS and the backward's scratch.
    Returns float32 [B].  A score is -inf, with zero gradients and never NaN, when T_b == 0, num_nodes < 1, nodes +
    arcs > max_states, an arc has src < 0, src >= dst or dst >= num_nodes, an arc is out of dst order, a label lies
    outside 0 .. C - 1, a weight is +inf or NaN, or no alignment fits.  Two paths that spell the same labels both count.
    The backward is one call that returns grad_out[b] * d score[b] / d log_probs and, when arc_weights requires a
    gradient, grad_out[b] * the posterior probability of every arc; it recomputes what it needs and sums in a fixed
    order without atomics, so it has the same bits run to run.  Runs on the caller's stream."""
    x = log_probs
    A, arcs_c, na, nn_, blank, frames, max_states = _lattice_args(
        "ctc_lattice_score", log_probs, arcs, num_arcs, num_nodes, arc_weights, blank, input_lengths, max_states)
    B = x.shape[0]
    if A == 0:
        # (an empty tensor has no address to hand over: one row that no count reaches stands in for none)
        out = _CTCLatticeScore.apply(x, None, arcs_c.new_zeros(B, 1, 3), torch.zeros_like(na), nn_, blank, frames,
                                     max_states)
        return out if arc_weights is None else out + (arc_weights.sum() * 0).to(out.dtype)  # (a gradient of zeros)
    return _CTCLatticeScore.apply(x, arc_weights, arcs_c, na, nn_, blank, frames, max_states)


def ctc_lattice_loss(log_probs, arcs, num_arcs, num_nodes, arc_weights=None, blank=0, input_lengths=None,
                     max_states=None):
    """The CTC criterion whose target is a token lattice: loss[b] = sum over t < T_b of logsumexp(log_probs[b, t]) -
    ctc_lattice_score(...)[b], float32 [B], differentiable in log_probs and arc_weights -- the negative log-likelihood
    of the lattice, marginalised over its paths (weighted by exp of their arc weights) and their alignments.  For a
    chain lattice without weights this is `ctc_loss`.  +inf where the score is -inf.  The arguments are those of
    `ctc_lattice_score`; rows past T_b are never read (their gradient is exactly 0)."""
    score = ctc_lattice_score(log_probs, arcs, num_arcs, num_nodes, arc_weights, blank, input_lengths, max_states)
    B, T, _ = log_probs.shape
    if input_lengths is None:
        return torch.logsumexp(log_probs, dim=2).sum(dim=1) - score
    frames = torch.as_tensor(_frame_counts("ctc_lattice_loss", input_lengths, B, T, 0), device=log_probs.device)
    inside = torch.arange(T, device=log_probs.device)[None, :] < frames[:, None]
    rows = torch.logsumexp(torch.where(inside[:, :, None], log_probs, torch.zeros_like(log_probs)), dim=2)
    return torch.where(inside, rows, torch.zeros_like(rows)).sum(dim=1) - score


def ctc_lattice_align(log_probs, arcs, num_arcs, num_nodes, arc_weights=None, blank=0, input_lengths=None,
                      max_states=None, max_path=None, return_token_scores=False, return_frames=False):
    """Which path of its token lattice the model chose for each utterance, and when each token of that path was spoken:
    the best (lattice path, alignment) pair -- the maximum over the lattice's paths p and the alignments of labels(p) of
    w(p) + the summed log_probs -- in one call, the lattices read where they lie on the device.  It is the max-plus
    partner of `ctc_lattice_score`: forced alignment with pronunciation variants or optional tokens, and the chosen
    word-piece decomposition after training with `ctc_lattice_loss`.
    log_probs, arcs, num_arcs, num_nodes, arc_weights (detached), blank, input_lengths and max_states are those of
    `ctc_lattice_score`; max_path (>= 1, default max(1, min(A, max_states))) is the width P of the path rows.
    Returns (scores, path_len, path_arcs, path_tokens, starts, ends[, token_scores][, frame_arcs]) on log_probs.device:
      scores        float32 [B]: the best w(p) + alignment score, -inf without a path;
      path_len      int32 [B]: the arcs on the best path, 0 without one; a path longer than P keeps its true length;
      path_arcs     int32 [B, P]: the arc indices in path order (the first P of a longer path);
      path_tokens   int32 [B, P]: their labels -- with path_len the layout `ctc_score`, `edit_distance` and
                    `ctc_token_align` take;
      starts, ends  int32 [B, P]: the first frame of each arc and one past its last (blank frames belong to no arc);
                    all four rows hold -1 at and past path_len and for an utterance without a path;
      token_scores  float32 [B, P] (return_token_scores): the sum of log_probs[b, t, label] over the arc's frames; -inf
                    where starts is -1;
      frame_arcs    int32 [B, T] (return_frames): the arc index of every frame, -1 on blank frames and from T_b on.
    An utterance has no path exactly where `ctc_lattice_score` gives -inf.  A one-node lattice has the empty path: a
    finite score and rows of -1.  Float32 max-plus arithmetic; of equal candidates the first in the forward recurrence's
    order wins (the state itself, the blank of the arc's source, the arcs entering it in ascending order): the same bits
    every time.  No autograd.  Runs on the caller's stream."""
    who = "ctc_lattice_align"
    if max_path is not None and int(max_path) < 1:
        raise ValueError(f"{who}: max_path must be at least 1")
    A, arcs_c, na, nn_, blank, frames, max_states = _lattice_args(
        who, log_probs, arcs, num_arcs, num_nodes, arc_weights, blank, input_lengths, max_states)
    P = max(1, min(A, max_states)) if max_path is None else int(max_path)
    x = log_probs.detach().contiguous()
    B, T, _ = x.shape
    w = None if arc_weights is None else arc_weights.detach().to(torch.float32).contiguous()
    if A == 0:
        # (an empty tensor has no address to hand over: one row that no count reaches stands in for none)
        A, arcs_c, na, w = 1, arcs_c.new_zeros(B, 1, 3), torch.zeros_like(na), None
    stream = _engine_stream(x.device)
    F = max(T, 1)  # (rows without an element are never written, but they need an address)
    scores = torch.empty(B, dtype=torch.float32, device=x.device)
    plen = torch.empty(B, dtype=torch.int32, device=x.device)
    rows = [torch.empty(B, P, dtype=torch.int32, device=x.device) for _ in range(4)]
    tsc = torch.empty(B, P, dtype=torch.float32, device=x.device) if return_token_scores else None
    fa = torch.empty(B, F, dtype=torch.int32, device=x.device) if return_frames else None
    if B == 0:
        _engine_done(stream)  # (no utterance: nothing to launch, and an empty tensor has no address to hand over)
    else:
        native = T == F and _has_native(who, "gtn_ctc_lattice_align_n")
        _route(stream, x, native, "gtn_ctc_lattice_align_n",
               (blank, _host_ptr(frames), arcs_c.data_ptr(), na.data_ptr(), nn_.data_ptr(), _ptr(w), A, max_states, P,
                scores.data_ptr(), plen.data_ptr(), *(r.data_ptr() for r in rows), _ptr(tsc), _ptr(fa)),
               "ctc_lattice_align", arcs_c.data_ptr(), na.data_ptr(), nn_.data_ptr(), scores.data_ptr(), plen.data_ptr(),
               *(r.data_ptr() for r in rows), _ptr(tsc), _ptr(fa), _ptr(w), frames, blank, max_states, A=A,
               row_stride=3 * A, P=P, out_stride=P, frame_stride=F)
    out = [scores, plen, *rows]
    if return_token_scores:
        out.append(tsc)
    if return_frames:
        out.append(fa[:, :T])
    return tuple(out)


class _ASGScore(torch.autograd.Function):
    """forward: one launch that stores nothing but the scores; backward: the one gradient call with grad_out as the
    weights, asked for the emission gradient and / or the table gradient as requires_grad says.  The node keeps tensors
    only: the backward recomputes what it needs."""

    @staticmethod
    def forward(ctx, emissions, transitions, start, tokens, lengths, frames, max_length):
        B, N, L = tokens.shape
        x = emissions.detach().contiguous()
        table = _asg_weights(start, transitions)
        stream = _engine_stream(x.device)
        scores = torch.empty(B, N, dtype=torch.float32, device=x.device)
        if B * N == 0:
            _engine_done(stream)  # (no pair: nothing to launch, and an empty tensor has no address to hand over)
        else:
            _route(stream, x, _has_native("asg_score", "gtn_asg_score_n"), "gtn_asg_score_n",
                   (table.data_ptr(), _host_ptr(frames), tokens.data_ptr(), lengths.data_ptr(), N, L, max_length,
                    scores.data_ptr()),
                   "asg_score", table.data_ptr(), tokens.data_ptr(), lengths.data_ptr(), scores.data_ptr(), frames,
                   max_length, N=N, L=L, row_stride=L)
        ctx.save_for_backward(x, table, tokens, lengths)
        ctx.args = (frames, max_length, transitions.dtype, start.dtype)
        return scores

    @staticmethod
    def backward(ctx, grad_out):
        x, table, tokens, lengths = ctx.saved_tensors
        frames, max_length, tr_dtype, st_dtype = ctx.args
        B, T, C_ = x.shape
        N, L = tokens.shape[1], tokens.shape[2]
        want_em = ctx.needs_input_grad[0]
        want_table = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if not (want_em or want_table):
            return (None,) * 7
        grad = torch.empty(B, T, C_, dtype=torch.float32, device=x.device) if want_em else None
        g_table = torch.empty(C_ + C_ * C_, dtype=torch.float32, device=x.device) if want_table else None
        if B * N == 0 or x.numel() == 0:
            for g in (grad, g_table):
                if g is not None:
                    g.zero_()
        else:
            w = grad_out.detach().to(torch.float32).contiguous()
            _route(_engine_stream(x.device), x, _native(), "gtn_asg_score_grad_n",
                   (table.data_ptr(), _host_ptr(frames), tokens.data_ptr(), lengths.data_ptr(), N, L, max_length,
                    w.data_ptr(), _ptr(grad), _ptr(g_table)),
                   "asg_score_grad", table.data_ptr(), tokens.data_ptr(), lengths.data_ptr(), w.data_ptr(), _ptr(grad),
                   _ptr(g_table), frames, max_length, N=N, L=L, row_stride=L)
        g_tr = g_table[C_:].reshape(C_, C_).to(tr_dtype) if ctx.needs_input_grad[1] else None
        g_st = g_table[:C_].to(st_dtype) if ctx.needs_input_grad[2] else None
        return grad, g_tr, g_st, None, None, None, None


def asg_score(emissions, transitions, tokens, lengths, start=None, input_lengths=None, max_length=None):
    """The ASG force-align term of device-resident hypotheses, differentiable: score[b, k] = forwardScore(emissions[b,
    :T_b] o (forceAlign(tokens[b, k, :len]) o transitions)), the log-sum over all alignments of the summed emissions, start
    and transition scores, for all B * N hypotheses in one launch against the B shared slabs -- no download of the tokens,
    no wait, no repeated emissions.  Nothing is subtracted: `asg_loss(x, tr, [y]) == fullConnect(x, tr) - asg_score(x, tr,
    y)`.  It is what rescoring an N-best list, a risk or margin objective over several hypotheses per utterance, and
    per-hypothesis weights on `transitions` and `start` need (`asg_decode(collapse=True)` -> `asg_score`).
    emissions: float32 CUDA tensor [B, T, C] (any scores), read in place; transitions: [C, C] with transitions[i, j] the
    score of label j followed by label i; start: [C] scores of the first label (zeros when omitted); tokens: int32 CUDA
    tensor [B, N, L] or [B, L] of labels (there is no blank; equal neighbours are legal, as in forceAlign); lengths: int32
    or int64 CUDA tensor [B, N] / [B], read on the device and clamped to 0 .. L there -- elements at or past a length are
    never read; input_lengths: per-utterance frame counts (0 .. T) or None -- rows past T_b are never read and their
    gradient is exactly 0; max_length (1 .. 4096, default min(L, T, 4096)): the caller's bound on the hypotheses'
    lengths, which sizes the kernel's LDS and the backward's scratch.  At most 16384 labels.
    Returns float32 [B, N] (or [B]).  A score is -inf, with zero gradient and never NaN, when the length is 0, T_b is
    below the length (T_b == 0 included), the length is above max_length, a token inside the length lies outside
    0 .. C - 1, or every alignment crosses a -inf emission, transition or start score.
    The backward is one call with grad_out as per-hypothesis weights; it returns gradients for emissions, transitions and
    start, computes only those that require grad, recomputes what it needs (the node keeps tensors only), skips pairs
    whose score is -inf or whose incoming gradient is exactly 0, and sums in a fixed order without atomics, so it has the
    same bits run to run.  A non-uniform grad_out is fine: this is the case `asg_loss(reduction="none")` refuses.  Without
    requires_grad it never launches.  Runs on the caller's stream."""
    def tables(C_):
        if not (torch.is_tensor(transitions) and tuple(transitions.shape) == (C_, C_)):
            raise ValueError(f"asg_score: transitions must be [{C_}, {C_}]")
        if start is not None and not (torch.is_tensor(start) and tuple(start.shape) == (C_,)):
            raise ValueError(f"asg_score: start must be [{C_}]")
        if C_ < 1 or C_ > 16384:
            raise ValueError("asg_score: the number of labels must be 1 .. 16384")
        return (transitions, "transitions"), (start, "start")
    B, _, C_, _, _, flat, tok, ln, frames, max_length = _hypothesis_args(
        "asg_score", "scores", emissions, "emissions", tokens, lengths, None, input_lengths, max_length, tables)
    if start is None:
        start = torch.zeros(C_, dtype=torch.float32, device=emissions.device)
    out = _ASGScore.apply(emissions, transitions, start, tok, ln, frames, max_length)
    return out.reshape(B) if flat else out


class _ASGLatticeScore(torch.autograd.Function):
    """forward: one launch that stores nothing but the scores; backward: the one gradient call with grad_out as the
    weights, asked for the emission, table and arc gradients as requires_grad says.  The node keeps tensors only."""

    @staticmethod
    def forward(ctx, emissions, transitions, start, arc_weights, arcs, num_arcs, num_nodes, frames, max_states, max_edges):
        B, A = arcs.shape[:2]
        x = emissions.detach().contiguous()
        table = _asg_weights(start, transitions)
        w = None if arc_weights is None else arc_weights.detach().to(torch.float32).contiguous()
        stream = _engine_stream(x.device)
        scores = torch.empty(B, dtype=torch.float32, device=x.device)
        if B == 0:
            _engine_done(stream)  # (no utterance: nothing to launch, and an empty tensor has no address to hand over)
        else:
            _route(stream, x, _has_native("asg_lattice_score", "gtn_asg_lattice_score_n"), "gtn_asg_lattice_score_n",
                   (table.data_ptr(), _host_ptr(frames), arcs.data_ptr(), num_arcs.data_ptr(), num_nodes.data_ptr(),
                    _ptr(w), A, max_states, max_edges, scores.data_ptr()),
                   "asg_lattice_score", table.data_ptr(), arcs.data_ptr(), num_arcs.data_ptr(), num_nodes.data_ptr(),
                   scores.data_ptr(), _ptr(w), frames, max_states, max_edges, A=A, row_stride=3 * A)
        ctx.save_for_backward(x, table, arcs, num_arcs, num_nodes, *(() if w is None else (w,)))
        ctx.args = (frames, max_states, max_edges, transitions.dtype, start.dtype,
                    None if arc_weights is None else arc_weights.dtype)
        return scores

    @staticmethod
    def backward(ctx, grad_out):
        x, table, arcs, num_arcs, num_nodes, *rest = ctx.saved_tensors
        w = rest[0] if rest else None
        frames, max_states, max_edges, tr_dtype, st_dtype, w_dtype = ctx.args
        B, T, C_ = x.shape
        A = arcs.shape[1]
        want_em = ctx.needs_input_grad[0]
        want_table = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        want_w = w is not None and ctx.needs_input_grad[3]
        none = (None,) * 6
        if not (want_em or want_table or want_w):
            return (None,) * 4 + none
        grad = torch.empty(B, T, C_, dtype=torch.float32, device=x.device) if want_em else None
        g_table = torch.empty(C_ + C_ * C_, dtype=torch.float32, device=x.device) if want_table else None
        garc = torch.empty(B, A, dtype=torch.float32, device=x.device) if want_w else None
        if B == 0 or x.numel() == 0:
            for g in (grad, g_table, garc):
                if g is not None:
                    g.zero_()
        else:
            g = grad_out.detach().to(torch.float32).contiguous()
            _route(_engine_stream(x.device), x, _native(), "gtn_asg_lattice_score_grad_n",
                   (table.data_ptr(), _host_ptr(frames), arcs.data_ptr(), num_arcs.data_ptr(), num_nodes.data_ptr(),
                    _ptr(w), A, max_states, max_edges, g.data_ptr(), _ptr(grad), _ptr(g_table), _ptr(garc)),
                   "asg_lattice_score_grad", table.data_ptr(), arcs.data_ptr(), num_arcs.data_ptr(),
                   num_nodes.data_ptr(), g.data_ptr(), _ptr(grad), _ptr(g_table), _ptr(garc), _ptr(w), frames,
                   max_states, max_edges, A=A, row_stride=3 * A)
        g_tr = g_table[C_:].reshape(C_, C_).to(tr_dtype) if ctx.needs_input_grad[1] else None
        g_st = g_table[:C_].to(st_dtype) if ctx.needs_input_grad[2] else None
        return (grad, g_tr, g_st, garc.to(w_dtype) if want_w else None) + none


def asg_lattice_score(emissions, transitions, arcs, num_arcs, num_nodes, arc_weights=None, start=None,
                      input_lengths=None, max_states=None, max_edges=None):
    """The exact ASG log score of one acyclic token lattice per utterance, differentiable: score[b] = log sum over the
    lattice's paths p of exp(w(p) + asg_score(emissions[b, :T_b], transitions, labels(p))) -- every word-piece
    decomposition, pronunciation or optional token the lattice holds and every alignment of each, marginalised in one
    launch; the lattices are read where they lie on the device.  Nothing is subtracted (`asg_lattice_loss` does that).
    emissions: float32 CUDA tensor [B, T, C] (any scores), read in place; transitions: [C, C] with transitions[i, j] the
    score of label j followed by label i; start: [C] scores of the first label (zeros when omitted); arcs, num_arcs,
    num_nodes, arc_weights and input_lengths are those of `ctc_lattice_score` (arcs sorted by dst; `gtn_amd.pack_lattices`
    gives this form) -- the states are the arcs: there is no blank and equal neighbouring labels are legal, as in
    `asg_score`.  max_states (1 .. 4096, default min(2 A + 1, 4096)): the caller's bound on nodes + arcs, the same
    argument as for `ctc_lattice_score`; max_edges (1 .. 2^21, default min(8 * max_states, 2^21)): the caller's bound on
    the edges, the sum over the arcs of the in-degree of their src -- the lattices live on the device and the backward
    sizes its scratch by this bound without a download.  At most 16384 labels.
    Returns float32 [B].  A score is -inf, with zero gradients and never NaN, when T_b == 0, num_nodes < 1, nodes + arcs
    > max_states, the lattice has more edges than max_edges, an arc or a weight is invalid as for `ctc_lattice_score`,
    no alignment fits (a one-node lattice has none: ASG has no empty alignment), or every alignment crosses a -inf
    emission, transition or start score.
    The backward is one call with grad_out as per-utterance weights; it returns gradients for emissions, transitions,
    start and arc_weights (grad_out[b] times the posterior of every arc), computes only those that require grad,
    recomputes what it needs and sums in a fixed order without atomics, so it has the same bits run to run.  Without
    requires_grad it never launches.  Runs on the caller's stream."""
    who = "asg_lattice_score"
    x = emissions
    if not (torch.is_tensor(x) and x.dim() == 3 and x.dtype == torch.float32):
        raise ValueError(f"{who}: emissions must be a float32 tensor [B, T, C]")
    B, T, C_ = x.shape
    if not (torch.is_tensor(transitions) and tuple(transitions.shape) == (C_, C_)):
        raise ValueError(f"{who}: transitions must be [{C_}, {C_}]")
    if start is not None and not (torch.is_tensor(start) and tuple(start.shape) == (C_,)):
        raise ValueError(f"{who}: start must be [{C_}]")
    if C_ < 1 or C_ > 16384:
        raise ValueError(f"{who}: the number of labels must be 1 .. 16384")
    if not (torch.is_tensor(arcs) and arcs.dtype == torch.int32 and arcs.dim() == 3 and arcs.shape[0] == B
            and arcs.shape[2] == 3):
        raise ValueError(f"{who}: arcs must be an int32 tensor [B, A, 3] for a batch of {B}")
    A = arcs.shape[1]
    for t, name in ((num_arcs, "num_arcs"), (num_nodes, "num_nodes")):
        if not (torch.is_tensor(t) and t.dtype in (torch.int32, torch.int64) and tuple(t.shape) == (B,)):
            raise ValueError(f"{who}: {name} must be an int32 or int64 tensor [{B}]")
    if arc_weights is not None and not (torch.is_tensor(arc_weights) and arc_weights.is_floating_point()
                                        and tuple(arc_weights.shape) == (B, A)):
        raise ValueError(f"{who}: arc_weights must be a floating-point tensor [{B}, {A}]")
    max_states = max(1, min(2 * A + 1, 4096)) if max_states is None else int(max_states)
    if not 1 <= max_states <= 4096:
        raise ValueError(f"{who}: max_states outside 1 .. 4096")
    max_edges = min(8 * max_states, 1 << 21) if max_edges is None else int(max_edges)
    if not 1 <= max_edges <= 1 << 21:
        raise ValueError(f"{who}: max_edges outside 1 .. 2^21")
    frames = None if input_lengths is None else _frame_counts(who, input_lengths, B, T, 0)
    for t, what in ((x, "emissions"), (transitions, "transitions"), (start, "start"), (arcs, "arcs"),
                    (num_arcs, "num_arcs"), (num_nodes, "num_nodes"), (arc_weights, "arc_weights")):
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"{who}: {what} must be a CUDA tensor (the scores are computed on the device)")
        if t.device != x.device:
            raise ValueError(f"{who}: all tensors must be on one device")
    if start is None:
        start = torch.zeros(C_, dtype=torch.float32, device=x.device)
    arcs_c = arcs.detach().contiguous()
    na = num_arcs.detach().to(torch.int32).contiguous()  # (int64 counts are converted on the device)
    nn_ = num_nodes.detach().to(torch.int32).contiguous()
    if A == 0:
        # (an empty tensor has no address to hand over: one row that no count reaches stands in for none)
        out = _ASGLatticeScore.apply(x, transitions, start, None, arcs_c.new_zeros(B, 1, 3), torch.zeros_like(na), nn_,
                                     frames, max_states, max_edges)
        return out if arc_weights is None else out + (arc_weights.sum() * 0).to(out.dtype)  # (a gradient of zeros)
    return _ASGLatticeScore.apply(x, transitions, start, arc_weights, arcs_c, na, nn_, frames, max_states, max_edges)


class _ASGFullConnect(torch.autograd.Function):
    """the full-connect half of _ASGLoss: the gradients come with the forward, for unit seeds"""

    @staticmethod
    def forward(ctx, emissions, transitions, start, reduction, frames):
        B, T, N = emissions.shape
        lib = _native()
        if not lib or not hasattr(lib, "gtn_asg_full_connect_n"):
            raise RuntimeError("asg_full_connect needs gtn_asg_full_connect_n in gtn_amd/lib/libgtn_criteria.so "
                               "(run __graft_entry__.build())")
        x = emissions.detach().contiguous()
        w = _asg_weights(start, transitions)
        stream = _engine_stream(x.device)
        out = torch.empty(B, dtype=torch.float32, device=x.device)
        gem = torch.empty(B, T, N, dtype=torch.float32, device=x.device) if ctx.needs_input_grad[0] else None
        need_tr = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        gtr = torch.empty(N + N * N, dtype=torch.float32, device=x.device) if need_tr else None
        if B == 0:
            if gtr is not None:
                gtr.zero_()
        else:
            _call("gtn_asg_full_connect_n", x.data_ptr(), B, T, N, w.data_ptr(), _host_ptr(frames), out.data_ptr(),
                  _ptr(gem), _ptr(gtr))
        _engine_done(stream)
        ctx.grads = (gem, gtr)
        ctx.shape = (B, T, N)
        ctx.reduction = reduction
        ctx.dtypes = (transitions.dtype, start.dtype)
        return out.mean() if reduction == "mean" else (out.sum() if reduction == "sum" else out)

    @staticmethod
    def backward(ctx, grad_out):
        B, T, N = ctx.shape
        gem, gtr = ctx.grads
        if ctx.reduction == "none":
            # the table gradient was summed over the batch with unit seeds: per-utterance seeds must be uniform
            scale_em = grad_out.reshape(B, 1, 1)
            scale_tr = grad_out.reshape(-1)[0] if gtr is not None and B else None
            if gtr is not None and B and not bool((grad_out == grad_out.reshape(-1)[0]).all()):
                raise RuntimeError("asg_full_connect(reduction='none'): transition gradients need a uniform upstream "
                                   "gradient; use reduction='sum' or 'mean'")
        else:
            scale_em = (grad_out / B if ctx.reduction == "mean" else grad_out).reshape(1, 1, 1)
            scale_tr = scale_em.reshape(())
        g_em = gem * scale_em if gem is not None and ctx.needs_input_grad[0] else None
        g_tr = g_st = None
        if gtr is not None:
            scaled = gtr * scale_tr if scale_tr is not None else gtr
            g_st = scaled[:N].to(ctx.dtypes[1]) if ctx.needs_input_grad[2] else None
            g_tr = scaled[N:].reshape(N, N).to(ctx.dtypes[0]) if ctx.needs_input_grad[1] else None
        return g_em, g_tr, g_st, None, None


def asg_full_connect(emissions, transitions, start=None, input_lengths=None, reduction="none"):
    """The full-connect term of the ASG criterion on its own, differentiable: score[b] = forwardScore(emissions[b, :T_b] o
    transitions), the log-sum over every label sequence and every alignment -- the normaliser `asg_loss` subtracts its
    force-align term from, for criteria with another numerator (`asg_lattice_loss`).  `asg_loss(x, tr, [y]) ==
    asg_full_connect(x, tr) - asg_score(x, tr, y)`.  It runs the launches `asg_loss` runs for this term and has its
    rules: emissions float32 CUDA [B, T, C]; transitions [C, C]; start [C] or None (zeros); input_lengths: frame counts
    1 .. T or None; reduction "none", "sum" or "mean".  The transitions and start gradients are summed over the batch
    with unit seeds, so under reduction="none" they need a uniform upstream gradient (a RuntimeError otherwise)."""
    who = "asg_full_connect"
    x = emissions
    if not (torch.is_tensor(x) and x.dim() == 3 and x.dtype == torch.float32):
        raise ValueError(f"{who}: emissions must be a float32 tensor [B, T, C]")
    B, T, C_ = x.shape
    if not (torch.is_tensor(transitions) and tuple(transitions.shape) == (C_, C_)):
        raise ValueError(f"{who}: transitions must be [{C_}, {C_}]")
    if start is not None and not (torch.is_tensor(start) and tuple(start.shape) == (C_,)):
        raise ValueError(f"{who}: start must be [{C_}]")
    if reduction not in ("none", "sum", "mean"):
        raise ValueError(f"{who}: reduction must be 'none', 'sum' or 'mean'")
    frames = None if input_lengths is None else _frame_counts(who, input_lengths, B, T, 1)
    for t, what in ((x, "emissions"), (transitions, "transitions"), (start, "start")):
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{who}: {what} must be a CUDA tensor (the scores are computed on the device)")
    if start is None:
        start = torch.zeros(C_, dtype=torch.float32, device=x.device)
    return _ASGFullConnect.apply(x, transitions, start, reduction, frames)


def asg_lattice_loss(emissions, transitions, arcs, num_arcs, num_nodes, arc_weights=None, start=None,
                     input_lengths=None, max_states=None, max_edges=None):
    """The ASG criterion whose target is a token lattice: loss[b] = asg_full_connect(...)[b] - asg_lattice_score(...)[b],
    float32 [B], differentiable in emissions, transitions, start and arc_weights -- the negative log-likelihood of the
    lattice, marginalised over its paths (weighted by exp of their arc weights) and their alignments.  For a chain
    lattice without weights this is `asg_loss`.  +inf where the score is -inf.  The arguments are those of
    `asg_lattice_score`, except that the frame counts are 1 .. T (the full-connect term's rule).  The full-connect term's
    table gradient needs a uniform upstream gradient: reduce the losses with .sum() or .mean()."""
    score = asg_lattice_score(emissions, transitions, arcs, num_arcs, num_nodes, arc_weights, start, input_lengths,
                              max_states, max_edges)
    return asg_full_connect(emissions, transitions, start, input_lengths) - score


def ctc_token_align(log_probs, tokens, lengths, blank=0, input_lengths=None, max_length=None, return_token_scores=False,
                    return_frames=False):
    """When each token of each device-resident hypothesis was spoken, and how well the frames support it: the best
    alignment (the reference's viterbiPath over ctcGraph(tokens[b, k, :len], blank) o log_probs[b, :T_b]) of all B * N
    hypotheses in one call against the B shared slabs -- no download of the tokens, no wait, no host loop over frames.
    It takes the tensors where `ctc_beam_decode` left them.
    log_probs, tokens ([B, N, L] or [B, L]), lengths (int32 or int64, clamped to 0 .. L on the device), blank,
    input_lengths and max_length (1 .. 4096, default min(L, T, 4096)) are those of `ctc_score`.
    Returns (scores, starts, ends[, token_scores][, frame_tokens]) on log_probs.device:
      scores        float32 [B, N] (or [B]): the score of the best path, -inf without one;
      starts, ends  int32 [B, N, L] (or [B, L]): the first frame of token i and one past its last, so ends - starts is
                    its duration (blank frames belong to no token); -1 for i >= len and for a pair without a path;
      token_scores  float32, same shape (return_token_scores): the sum of log_probs[b, t, token] over the token's
                    frames; -inf where starts is -1.  With normalised log_probs exp(token_scores / (ends - starts)) is
                    the usual per-token confidence; nothing is subtracted here;
      frame_tokens  int32 [B, N, T] (or [B, T]) (return_frames): the token index of every frame, -1 on blank frames and
                    from T_b on -- the `tokens` plane of `ctc_forced_align`.
    A pair has no path where `ctc_score` gives -inf: length + repeats > T_b, every path crosses a -inf emission, the
    length is above max_length, a token inside the length is outside 0 .. C - 1, T_b == 0.  A beam slot without a
    hypothesis (length 0) aligns as the empty sequence: a finite score and rows of -1.  Float32 max-plus arithmetic with
    exact ties decided as `ctc_forced_align` decides them: the same bits every time.  No autograd.  Runs on the caller's
    stream."""
    blank = int(blank)
    B, T, _, N, L, flat, tok, ln, frames, max_length = _hypothesis_args(
        "ctc_token_align", "alignments", log_probs, "log_probs", tokens, lengths, blank, input_lengths, max_length)
    x = log_probs.detach().contiguous()
    stream = _engine_stream(x.device)
    # (rows without an element are never written, but they need an address: a width of at least 1 behind the views)
    W, F = max(L, 1), max(T, 1)
    scores = torch.empty(B, N, dtype=torch.float32, device=x.device)
    starts = torch.empty(B, N, W, dtype=torch.int32, device=x.device)
    ends = torch.empty(B, N, W, dtype=torch.int32, device=x.device)
    tsc = torch.empty(B, N, W, dtype=torch.float32, device=x.device) if return_token_scores else None
    ftk = torch.empty(B, N, F, dtype=torch.int32, device=x.device) if return_frames else None
    if tok.numel() == 0:
        tok = tok.new_empty(B, N, 1)
    if B * N == 0:
        _engine_done(stream)  # (no pair: nothing to launch, and an empty tensor has no address to hand over)
    else:
        native = L == W and T == F and _has_native("ctc_token_align", "gtn_ctc_token_align_n", python_route=True)
        _route(stream, x, native, "gtn_ctc_token_align_n",
               (blank, _host_ptr(frames), tok.data_ptr(), ln.data_ptr(), N, L, max_length, scores.data_ptr(),
                starts.data_ptr(), ends.data_ptr(), _ptr(tsc), _ptr(ftk)),
               "ctc_token_align", tok.data_ptr(), ln.data_ptr(), scores.data_ptr(), starts.data_ptr(), ends.data_ptr(),
               _ptr(tsc), _ptr(ftk), frames, blank, max_length, N=N, L=L, row_stride=W, out_stride=W, frame_stride=F)
    out = [scores, starts[:, :, :L], ends[:, :, :L]]
    if return_token_scores:
        out.append(tsc[:, :, :L])
    if return_frames:
        out.append(ftk[:, :, :T])
    if flat:
        out = [o.reshape(B, *o.shape[2:]) for o in out]
    return tuple(out)


def asg_token_align(emissions, transitions, tokens, lengths, start=None, input_lengths=None, max_length=None,
                    return_token_scores=False, return_frames=False):
    """When each token of each device-resident ASG hypothesis was spoken, and how well the frames support it: the best
    alignment (the reference's viterbiPath over emissions[b, :T_b] o (forceAlign(tokens[b, k, :len]) o transitions)) of
    all B * N hypotheses in one call against the B shared slabs -- no download of the tokens, no wait, no host loop over
    frames.  It takes the tensors where `asg_beam_decode` or `asg_decode(collapse=True)` left them.
    emissions, transitions, start, tokens ([B, N, L] or [B, L]), lengths (int32 or int64, clamped to 0 .. L on the
    device), input_lengths and max_length (1 .. 4096, default min(L, T, 4096)) are those of `asg_score`; transitions and
    start are detached.  There is no cap on the number of labels of this call's own.
    Returns (scores, starts, ends[, token_scores][, frame_tokens]) on emissions.device:
      scores        float32 [B, N] (or [B]): the score of the best path (emissions, start and transitions), -inf without
                    one;
      starts, ends  int32 [B, N, L] (or [B, L]): the first frame of token i and one past its last; with a path starts[0]
                    is 0, ends[i] is starts[i + 1] and ends[len - 1] is T_b; -1 for i >= len and for a pair without a
                    path;
      token_scores  float32, same shape (return_token_scores): the sum of emissions[b, t, token] over the token's frames,
                    emissions only; -inf where starts is -1.  With normalised emissions exp(token_scores / (ends -
                    starts)) is the same per-token confidence as `ctc_token_align`'s;
      frame_tokens  int32 [B, N, T] (or [B, T]) (return_frames): the token index of every frame, never -1 inside a path,
                    -1 from T_b on -- the `tokens` plane of `asg_forced_align`.
    A pair has no path exactly where `asg_score` gives -inf: the length is 0 (a beam slot without a hypothesis), T_b is
    below the length, the length is above max_length, a token inside the length is outside 0 .. C - 1, or every
    alignment crosses a -inf emission, transition or start score.  Float32 max-plus with the arithmetic of
    `asg_forced_align` (its scores and tokens bit for bit where both apply); of two exactly equal candidates the step
    wins: the same bits every time.  No autograd.  Runs on the caller's stream and does not wait."""
    def tables(C_):
        if not (torch.is_tensor(transitions) and tuple(transitions.shape) == (C_, C_)):
            raise ValueError(f"asg_token_align: transitions must be [{C_}, {C_}]")
        if start is not None and not (torch.is_tensor(start) and tuple(start.shape) == (C_,)):
            raise ValueError(f"asg_token_align: start must be [{C_}]")
        if C_ < 1:
            raise ValueError("asg_token_align: no labels")
        return (transitions, "transitions"), (start, "start")
    B, T, C_, N, L, flat, tok, ln, frames, max_length = _hypothesis_args(
        "asg_token_align", "alignments", emissions, "emissions", tokens, lengths, None, input_lengths, max_length, tables)
    x = emissions.detach().contiguous()
    # (written on the caller's stream BEFORE the engine is pointed at it, as in asg_beam_decode)
    st = torch.zeros(C_, dtype=torch.float32, device=x.device) if start is None else start
    table = _asg_weights(st, transitions)
    stream = _engine_stream(x.device)
    # (rows without an element are never written, but they need an address: a width of at least 1 behind the views)
    W, F = max(L, 1), max(T, 1)
    scores = torch.empty(B, N, dtype=torch.float32, device=x.device)
    starts = torch.empty(B, N, W, dtype=torch.int32, device=x.device)
    ends = torch.empty(B, N, W, dtype=torch.int32, device=x.device)
    tsc = torch.empty(B, N, W, dtype=torch.float32, device=x.device) if return_token_scores else None
    ftk = torch.empty(B, N, F, dtype=torch.int32, device=x.device) if return_frames else None
    if tok.numel() == 0:
        tok = tok.new_empty(B, N, 1)
    if B * N == 0:
        _engine_done(stream)  # (no pair: nothing to launch, and an empty tensor has no address to hand over)
    else:
        native = L == W and T == F and _has_native("asg_token_align", "gtn_asg_token_align_n")
        _route(stream, x, native, "gtn_asg_token_align_n",
               (table.data_ptr(), _host_ptr(frames), tok.data_ptr(), ln.data_ptr(), N, L, max_length, scores.data_ptr(),
                starts.data_ptr(), ends.data_ptr(), _ptr(tsc), _ptr(ftk)),
               "asg_token_align", tok.data_ptr(), ln.data_ptr(), scores.data_ptr(), starts.data_ptr(), ends.data_ptr(),
               _ptr(tsc), _ptr(ftk), frames, table.data_ptr(), max_length, N=N, L=L, row_stride=W, out_stride=W,
               frame_stride=F)
    out = [scores, starts[:, :, :L], ends[:, :, :L]]
    if return_token_scores:
        out.append(tsc[:, :, :L])
    if return_frames:
        out.append(ftk[:, :, :T])
    if flat:
        out = [o.reshape(B, *o.shape[2:]) for o in out]
    return tuple(out)
