"""The create refusals of the four small handle families (ffe_nstep_*, ffe_sampler_*, ffe_eplog_*, ffe_walktask_*) that are decided
before any device is needed, through ctypes on the built library: every one returns -1, leaves *out NULL and leaves its text in the
family's `last_error(NULL)`.  `PARENT` is what the library said before the families moved onto the shared handle layer
(csrc/handle.hpp), recorded by running these same calls on it; the texts are unchanged except where the n-step family had none or
had no prefix (include/flybody_env.h) - there the old text is a suffix of the new one."""
import ctypes as C

SENTINEL = 0xDEAD0

# case -> the text of the library before the change
PARENT = {
    "nstep null out": "",
    "nstep batch 0": "ffe_nstep_create: bad arguments",
    "nstep capacity below batch x n_step": "ffe_nstep_create: capacity 7 is below batch x n_step = 8, the rows one call can write: they would share slots of the ring",
    "nstep no device": "no such HIP device: the MI355X path has no CPU fallback",
    "nstep tracked no device": "no such HIP device: the MI355X path has no CPU fallback",
    "eplog null out": "ffe_eplog_create: null out",
    "eplog capacity below batch": "ffe_eplog_create: capacity 7 is below batch = 8, the records one call can write: they would share slots of the ring",
    "eplog batch 0": "ffe_eplog_create: batch 0 is below 1",
    "eplog unknown flags": "ffe_eplog_create: unknown flags 2",
    "eplog no device": "ffe_eplog_create: no such HIP device: the MI355X path has no CPU fallback",
    "sampler null out": "ffe_sampler_create: null out",
    "sampler null writers": "ffe_sampler_create: null writers",
    "sampler n_writers 0": "ffe_sampler_create: n_writers 0 is outside 1 .. 8",
    "sampler n_writers 9": "ffe_sampler_create: n_writers 9 is outside 1 .. 8",
    "sampler batch 0": "ffe_sampler_create: batch 0 is outside 1 .. 2^20",
    "sampler min_size 0": "ffe_sampler_create: min_size 0 is below 1",
    "sampler unknown flags": "ffe_sampler_create: unknown flags 2",
    "sampler null writer": "ffe_sampler_create: writer 0 is null",
    "walktask null out": "ffe_walktask_create: a null required pointer (out)",
    "walktask unknown flags": "ffe_walktask_create: unknown flags 2",
    "walktask no device": "ffe_walktask_create: no such HIP device: the MI355X path has no CPU fallback",
}
# the n-step family's additions: no text before / no prefix before
CHANGED = {
    "nstep null out": "ffe_nstep_create: null out",
    "nstep no device": "ffe_nstep_create: no such HIP device: the MI355X path has no CPU fallback",
    "nstep tracked no device": "ffe_nstep_create: no such HIP device: the MI355X path has no CPU fallback",
}


def cases(L):
    """[(case, family's last_error, call(out) -> rc)]; `out` is a byref to the handle slot.  A sampler cannot get as far as its
    device check without a writer, and a writer needs a device: its last case is a NULL entry in a valid argument list."""
    from flybody_amd.batched_env import WALK_BLOB
    from flybody_amd.tasks.walk_tracker import make_task
    from flybody_amd.tasks.walking import WalkModelView

    task, keep = make_task(WalkModelView())
    blob = open(WALK_BLOB, "rb").read()
    no_writers = (C.c_void_p * 9)()
    ne, se, le, we = L.ffe_nstep_last_error, L.ffe_sampler_last_error, L.ffe_eplog_last_error, L.ffe_walktask_last_error
    sampler = lambda w, n, batch, min_size, flags: (lambda out: L.ffe_sampler_create(w, n, batch, 0, min_size, flags, 0, out))  # noqa: E731
    walktask = lambda flags: (lambda out: L.ffe_walktask_create(blob, len(blob), C.byref(task), flags, 0, out))  # noqa: E731
    return keep, [
        ("nstep null out", ne, lambda out: L.ffe_nstep_create(2, 3, 2, 2, 0.99, 4, 0, None)),
        ("nstep batch 0", ne, lambda out: L.ffe_nstep_create(0, 3, 2, 2, 0.99, 4, 0, out)),
        ("nstep capacity below batch x n_step", ne, lambda out: L.ffe_nstep_create(4, 3, 2, 2, 0.99, 7, 0, out)),
        ("nstep no device", ne, lambda out: L.ffe_nstep_create(2, 3, 2, 2, 0.99, 4, 0, out)),
        ("nstep tracked no device", ne, lambda out: L.ffe_nstep_create_tracked(2, 3, 2, 2, 0.99, 4, 0, out)),
        ("eplog null out", le, lambda out: L.ffe_eplog_create(4, 4, 0, 0, None)),
        ("eplog capacity below batch", le, lambda out: L.ffe_eplog_create(8, 7, 0, 0, out)),
        ("eplog batch 0", le, lambda out: L.ffe_eplog_create(0, 4, 0, 0, out)),
        ("eplog unknown flags", le, lambda out: L.ffe_eplog_create(4, 4, 2, 0, out)),
        ("eplog no device", le, lambda out: L.ffe_eplog_create(4, 4, 0, 0, out)),
        ("sampler null out", se, lambda out: L.ffe_sampler_create(no_writers, 1, 4, 0, 1, 0, 0, None)),
        ("sampler null writers", se, sampler(None, 1, 4, 1, 0)),
        ("sampler n_writers 0", se, sampler(no_writers, 0, 4, 1, 0)),
        ("sampler n_writers 9", se, sampler(no_writers, 9, 4, 1, 0)),
        ("sampler batch 0", se, sampler(no_writers, 1, 0, 1, 0)),
        ("sampler min_size 0", se, sampler(no_writers, 1, 4, 0, 0)),
        ("sampler unknown flags", se, sampler(no_writers, 1, 4, 1, 2)),
        ("sampler null writer", se, sampler(no_writers, 1, 4, 1, 0)),
        ("walktask null out", we, lambda out: L.ffe_walktask_create(blob, len(blob), C.byref(task), 0, 0, None)),
        ("walktask unknown flags", we, walktask(2)),
        ("walktask no device", we, walktask(0)),
    ]


def run(L):
    """{case: (rc, *out afterwards, text)} in the order of `cases`"""
    keep, table = cases(L)
    got = {}
    for name, last_error, call in table:
        out = C.c_void_p(SENTINEL)
        rc = call(C.byref(out))
        got[name] = (rc, out.value, last_error(None).decode())
        if rc == 0:  # a machine with a device 0: the valid argument lists make handles
            getattr(L, last_error.__name__.replace("last_error", "destroy"))(out)
    del keep
    return got


def test_create_refusals_keep_their_texts():
    import torch

    from flybody_amd import _capi, build

    build.build()
    got = run(_capi.lib())
    assert list(got) == list(PARENT)
    for name, (rc, out, text) in got.items():
        print(name, rc, out, repr(text))
        if torch.cuda.is_available() and name.endswith("no device"):  # device 0 exists: the call succeeds (and is covered on the GPU)
            continue
        assert rc == -1, (name, rc)
        assert out == (SENTINEL if name.endswith("null out") else None), (name, out)  # no slot to clear when `out` itself is NULL
        if name in CHANGED:
            assert text == CHANGED[name] and text.endswith(PARENT[name]), (name, text)
        else:
            assert text == PARENT[name], (name, text)
