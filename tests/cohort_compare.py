"""How an evaluation of the cohort unit is compared with the model (tests/cohort_model.py): used by tests/test_cohort_gpu.py on
what the kernels give and by tests/test_cohort_model.py on dictionaries that never saw a GPU (the model itself, and
deliberately wrong variants of it, which same() has to reject).

Two comparisons.  The project's tolerance for these outputs, 1e-6 absolute against the float64 model, as before.  And one
that sees the small numbers -- f down to 1e-10, counts of 1e-30, most of r -- against the model in long double: f, count, r
and post RELATIVELY wherever the reference is at least FLOOR = 2^-1000 (below it absolutely against FLOOR: flushes and the
underflow of exp at the denormal edge are not the subject); logZ and both trace columns absolutely, since a sum of logs can
pass through zero and the second column is a difference of two f.

The tolerances.  S_OUT is, per output, the spread of the reference itself: the largest such difference between the float64
sequential model and the long-double one, measured on the CPU over everything cohort_cases.compared() yields -- the golden
cohort at the GPU tests' parameter sets, every item of CASES and TIES, the batch of nine, the classes of the big call,
small_item(2) at 4 096 iterations --, with the room said at S_OUT (tests/test_cohort_model.py measures it again on every
run and asserts it stays within).  The device gets FACTOR = 64 times that: it sums in another order than either evaluation
(butterflies, then (0 + 1) + (2 + 3)), its exp, log and division are within an ulp or two of numpy's and not equal to them,
and both compound through the iterations as the float64 / long-double difference does -- two to three bits per source,
three sources.  The relative tolerances have to stay at or below REL_CAP = 1e-10, two orders below the smallest slip worth
catching (single precision anywhere in the chain, 6e-8 or more): a case that needs more is ill-conditioned and is to be
replaced, not the cap raised."""
import numpy as np

from . import cohort_model as cm

assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is no wider than double here: there is no reference"

TOL = 1e-6
FLOOR = 2.0 ** -1000
FACTOR, REL_CAP = 64, 1e-10
RELATIVE, ABSOLUTE = ("f", "count", "r", "post"), ("logZ", "trace logZ", "trace delta")
# measured as said above (x86-64, glibc's libm, numpy 2.2): f 2.1e-14, count 2.3e-14, r 4.7e-14, post 1.1e-14 relative (all
# but post on the golden cohort at alpha 1e-6, 64 iterations), logZ 1.8e-14, trace logZ 6.2e-12, trace delta 5.8e-15 absolute
# (sums over the 685 samples of two_chunks_plus_5); each the next power of two above twice the figure -- another libm, or
# another SIMD path of numpy's exp, moves the figures by tens of per cent
S_OUT = {"f": 2.0 ** -44, "count": 2.0 ** -44, "r": 2.0 ** -43, "post": 2.0 ** -45, "logZ": 2.0 ** -44, "trace logZ": 2.0 ** -36,
         "trace delta": 2.0 ** -46}
TOLERANCE = {name: FACTOR * s for name, s in S_OUT.items()}
OBSERVED = {}            # the largest difference per output over everything same() has seen, for the module's last line


def difference(name, got, ref):
    """The largest difference of an output from the reference, relative or absolute as its name says, as a float."""
    if not np.size(ref):
        return 0.0
    got, ref = np.asarray(got, np.longdouble), np.asarray(ref, np.longdouble)
    d = np.abs(got - ref)
    if name in RELATIVE:
        d = d / np.maximum(ref, FLOOR)
    return float(d.max())


def outputs_of(x):
    """(name, values) of every compared output of a model's dict (samples that take no part left out)."""
    some = [s for s in range(len(x["call"])) if x["call"][s] is not None]
    return [("f", x["freq"]), ("count", x["count"]), ("trace logZ", x["trace"][:, 0]), ("trace delta", x["trace"][:, 1]),
            ("logZ", np.array([x["logZ"][s] for s in some], np.longdouble)), ("post", np.array([x["post"][s] for s in some], np.longdouble)),
            ("r", np.concatenate([np.asarray(x["r"][s], np.longdouble) for s in some] + [np.zeros(0, np.longdouble)]))]


def spread(want, ref):
    """{output: difference} between two evaluations of the model: what S_OUT is measured with."""
    return {name: difference(name, w, r) for (name, w), (_, r) in zip(outputs_of(want), outputs_of(ref))}


def from_model(x):
    """A model's dict in the form of one item of a Context.cohort call, as same() takes it: float64 arrays, no spare room."""
    ns = len(x["call"])
    call, values = np.zeros((ns, 3), np.int32), np.zeros((ns, 2))
    for s in range(ns):
        if x["call"][s] is not None:
            call[s] = (x["index"][s],) + x["call"][s]
            values[s] = (x["logZ"][s], x["post"][s])
    return dict(status=x["status"], A=len(x["alleles"]), alleles=x["alleles"], freq=np.asarray(x["freq"], np.float64),
                count=np.asarray(x["count"], np.float64), trace=np.asarray(x["trace"], np.float64), call=call, values=values,
                r=[np.zeros(0) if r is None else np.asarray(r, np.float64) for r in x["r"]])


def reference(samples, ploidy, **params):
    """The float64 model and the long-double one of an item."""
    return cm.evaluate(samples, ploidy, **params), cm.evaluate(samples, ploidy, dtype=np.longdouble, **params)


def _seen(name, diff):
    OBSERVED[name] = max(OBSERVED.get(name, 0.0), float(diff))


def _close(name, got, want, ref, what, relative):
    d = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max()) if np.size(want) else 0.0
    _seen(name, d)
    assert d <= TOL, (what, name, d)
    if relative:
        d = difference(name, got, ref)
        _seen(name + (" (relative)" if name in RELATIVE else " (long double)"), d)
        assert d <= TOLERANCE[name], (what, name, d, TOLERANCE[name])


def same(got, want, ref, what="", ties=False, relative=True):
    """One item of a call against the model's dict `want` (statuses, the support, the calls, 1e-6 absolute) and the
    long-double model's `ref` (the relative comparison; relative=False leaves it out: the comparison as it was).  ties:
    the item has exact ties by design, and what has to exceed 1e-5 is the distance in log q from the call to the best pair
    outside its tied group."""
    assert got["status"] == want["status"] == ref["status"], what
    if want["status"] != cm.OK:
        assert got["A"] == 0 and not got["alleles"].any() and not got["freq"].any() and not got["count"].any(), what
        assert not got["trace"].any() and not got["call"].any() and not got["values"].any(), what
        assert all(not r.any() for r in got["r"]), what
        return
    A = len(want["alleles"])
    assert got["A"] == A and np.array_equal(got["alleles"][:A], want["alleles"]) and np.array_equal(ref["alleles"], want["alleles"]), what
    assert not got["alleles"][A:].any() and not got["freq"][A:].any() and not got["count"][A:].any(), what
    _close("f", got["freq"][:A], want["freq"], ref["freq"], what, relative)
    _close("count", got["count"][:A], want["count"], ref["count"], what, relative)
    _close("trace logZ", got["trace"][:, 0], want["trace"][:, 0], ref["trace"][:, 0], what, relative)
    _close("trace delta", got["trace"][:, 1], want["trace"][:, 1], ref["trace"][:, 1], what, relative)
    for s in range(len(want["call"])):
        if want["call"][s] is None:                                 # a sample that takes no part: zeros
            assert not got["call"][s].any() and not got["values"][s].any() and len(got["r"][s]) == 0, (what, s)
            continue
        assert want["beyond" if ties else "gap"][s] > 1e-5, (what, s)          # every case has a call to compare
        assert tuple(got["call"][s].tolist()) == (want["index"][s],) + want["call"][s], (what, s)
        _close("logZ", got["values"][s, 0], want["logZ"][s], ref["logZ"][s], what, relative)
        _close("post", got["values"][s, 1], want["post"][s], ref["post"][s], what, relative)
        _close("r", got["r"][s], want["r"][s], ref["r"][s], what, relative)
