"""What the device encoders of variable-length output (training/png.py, training/jpeg.py) share on the host: the read-back of their streams
and the writing of the finished files."""

import os

import torch

_pinned = {}          # bytes -> pinned staging buffer of that (rounded-up) size


def _pinned_buffer(nbytes):
    size = 1 << max(16, (nbytes - 1).bit_length())
    buf = _pinned.get(size)
    if buf is None:
        buf = _pinned[size] = torch.empty([size], dtype=torch.uint8).pin_memory()
    return buf[:nbytes]


def streams_to_host(out, offsets):
    """(out uint8, offsets int64 [N + 1]) of a stream encoder on the device -> list of N `bytes`, stream k = out[offsets[k]:offsets[k + 1]].
    Two copies through a pinned buffer, each followed by a synchronisation of the current stream: the offsets, then the used bytes."""
    stream = torch.cuda.current_stream(out.device)
    head = _pinned_buffer(offsets.numel() * 8).view(torch.int64)
    head.copy_(offsets, non_blocking=True)
    stream.synchronize()
    ends = head.tolist()
    host = _pinned_buffer(max(ends[-1], 1))[:ends[-1]]          # no stream has a byte: a buffer of one byte, none of them used
    host.copy_(out[:ends[-1]], non_blocking=True)
    stream.synchronize()
    raw = host.numpy().tobytes()
    return [raw[ends[i]:ends[i + 1]] for i in range(len(ends) - 1)]


def write_files(files, paths, what):
    """files[k] -> paths[k] (one path for a single file); `what` names the caller in the error."""
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    if len(files) != len(paths):
        raise ValueError(f'{what}: {len(files)} frames for {len(paths)} paths')
    for data, path in zip(files, paths):
        with open(path, 'wb') as f:
            f.write(data)
