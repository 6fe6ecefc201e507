"""The output files' text, the reference's way: per read ">id\\n", then "<value> " per character and "\\n"
(shared by tests/test_gpu_text.py and tests/handle_steps.py)."""


def _expect(values, offs, ids):
    out = bytearray()
    for q, name in enumerate(ids):
        out += b">" + name + b"\n"
        out += b"".join(b"%d " % int(v) for v in values[offs[q]: offs[q + 1]]) + b"\n"
    return bytes(out)


def _fill(text, line_start, ids):
    b = bytearray(text)
    for q, name in enumerate(ids):
        at = int(line_start[q])
        b[at: at + len(name) + 2] = b">" + name + b"\n"
    return bytes(b)
