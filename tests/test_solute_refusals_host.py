"""CPU test: what the insertion and solute calls refuse without a device, as a table.

Every row is one call with a NULL batch and one or two bad arguments; its (status, mmc_last_error())
must equal the recorded row of tests/golden/solute_refusals.json, so a refusal keeps its status, its
text and its place in the order of checks -- also where two arguments are wrong at once -- and the
outputs come back untouched (the sentinels of the `call` helpers).  The file is written by this module,

    PYTHONPATH=. python tests/test_solute_refusals_host.py --record

and is only to be recorded again where a refusal is meant to change."""
import ctypes as C
import json
import os

import pytest

from metropolismontecarlo_amd import _lib
from test_solute_abi import call as solute_call
from test_solute_chain_abi import set_solute as set_solute_call
from test_solute_pair_abi import call as pair_call

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solute_refusals.json")
NAN, INF = float("nan"), float("inf")


def _arr(v, n):
    if v is None:
        return None
    vals = list(v) if isinstance(v, (tuple, list)) else [v] * n
    return (C.c_double * max(len(vals), 1))(*vals)


def _message(L):
    msg = L.mmc_last_error()
    return msg.decode() if msg else ""


def widom_call(at=False, offsets=0.5, mol=1.0, n_insert=4, temperature=298.15, sums=(True, True)):
    """One mmc_batch_widom / _widom_at with a NULL batch and sentinel outputs, which must come back
    untouched.  Returns (status, message)."""
    bs = (C.c_double * 4)(*([7.5] * 4))
    no = (C.c_int64 * 4)(*([3] * 4))
    du = (C.c_double * 64)(*([7.5] * 64))
    ov = (C.c_uint8 * 16)(*([9] * 16))
    mo = (C.c_double * 256)(*([7.5] * 256))
    L = _lib.lib()
    sm = (bs if sums[0] else None, no if sums[1] else None)
    if at:
        st = L.mmc_batch_widom_at(None, n_insert, _arr(mol, 12 * 4), temperature, *sm, du, ov)
    else:
        st = L.mmc_batch_widom(None, n_insert, 1234, 0, _arr(offsets, 9), temperature, *sm, mo, du, ov)
    assert all(v == 7.5 for v in bs) and all(v == 3 for v in no) and all(v == 7.5 for v in du)
    assert all(v == 9 for v in ov) and all(v == 7.5 for v in mo)
    return st, _message(L)


def deletion_call(temperature=298.15):
    """One mmc_batch_deletion of every molecule with a NULL batch and sentinel outputs."""
    es = (C.c_double * 16)(*([7.5] * 16))
    bs = (C.c_double * 4)(*([7.5] * 4))
    nf = (C.c_int64 * 4)(*([3] * 4))
    L = _lib.lib()
    st = L.mmc_batch_deletion(None, 0, None, temperature, 0, 0.0, 0.0, 0, None, es, bs, nf, None, None)
    assert all(v == 7.5 for v in es) and all(v == 7.5 for v in bs) and all(v == 3 for v in nf)
    return st, _message(L)


BAD6 = lambda i, v: tuple(v if j == i else 1.0 for j in range(6))  # noqa: E731  (two sites x three slots)

# what is wrong with one solute (S = 2), by the keywords of solute_call and set_solute_call
SOLUTE_FAULTS = {
    "n_sites=0": dict(n_sites=0), "n_sites=17": dict(n_sites=17),
    "charge=NULL": dict(charge=None), "eps=NULL": dict(eps=None), "sig=NULL": dict(sig=None),
    "charge=nan": dict(charge=(0.4, NAN)), "charge=inf": dict(charge=(INF, 0.0)),
    "eps=nan": dict(eps=NAN), "eps=inf": dict(eps=BAD6(4, INF)), "eps<0": dict(eps=BAD6(4, -1e-300)),
    "sig=nan": dict(sig=BAD6(0, NAN)), "sig=inf": dict(sig=INF), "sig<0": dict(sig=BAD6(5, -3.0)),
}
INSERT_FAULTS = {
    "n_insert=0": dict(n_insert=0), "temperature=0": dict(temperature=0.0), "temperature=nan": dict(temperature=NAN),
    "boltz_sum=NULL": dict(sums=(False, True)), "n_overlap=NULL": dict(sums=(True, False)),
}
OFFSETS_FAULTS = {"offsets=NULL": dict(offsets=None), "offsets=nan": dict(offsets=NAN),
                  "offsets=inf": dict(offsets=BAD6(4, -INF))}
MOL_FAULTS = {"mol=NULL": dict(mol=None), "mol=nan": dict(mol=NAN), "mol=inf": dict(mol=INF)}

# ... and with the pair (S_A = 2, S_B = 1), by the keywords of pair_call
PAIR_FAULTS = {
    "n_sites_a=0": dict(n_sites_a=0), "n_sites_a=17": dict(n_sites_a=17), "n_sites_b=0": dict(n_sites_b=0),
    "n_sites_b=17": dict(n_sites_b=17), "n_sites=15+2": dict(n_sites_a=15, n_sites_b=2), "n_sep=0": dict(K=0),
    "n_insert=0": dict(n_insert=0), "temperature=0": dict(temperature=0.0), "temperature=nan": dict(temperature=NAN),
    "eps_ab=NULL": dict(eps_ab=None), "sig_ab=NULL": dict(sig_ab=None),
    "eps_ab=nan": dict(eps_ab=(1.0, NAN)), "sig_ab<0": dict(sig_ab=(-0.5, 1.0)),
}
for _t, _n in (("a", 6), ("b", 3)):
    _bad = lambda i, v, n=_n: tuple(v if j == i else 1.0 for j in range(n))  # noqa: E731
    PAIR_FAULTS.update({
        f"charge_{_t}=NULL": {f"charge_{_t}": None}, f"eps_{_t}=NULL": {f"eps_{_t}": None},
        f"sig_{_t}=NULL": {f"sig_{_t}": None},
        f"charge_{_t}=nan": {f"charge_{_t}": (NAN,) * (_n // 3)}, f"charge_{_t}=inf": {f"charge_{_t}": (-INF,) * (_n // 3)},
        f"eps_{_t}=nan": {f"eps_{_t}": _bad(1, NAN)}, f"eps_{_t}=inf": {f"eps_{_t}": INF},
        f"eps_{_t}<0": {f"eps_{_t}": _bad(2, -1e-300)},
        f"sig_{_t}=nan": {f"sig_{_t}": NAN}, f"sig_{_t}=inf": {f"sig_{_t}": _bad(0, INF)},
        f"sig_{_t}<0": {f"sig_{_t}": _bad(2, -3.0)},
    })
PAIR_DRAWN_FAULTS = {
    "offsets_a=NULL": dict(offsets_a=None), "offsets_b=NULL": dict(offsets_b=None), "offsets_a=nan": dict(offsets_a=NAN),
    "offsets_b=inf": dict(offsets_b=(0.0, -INF, 0.0)), "d=NULL": dict(d=None), "d=nan": dict(d=(3.0, NAN)),
    "d=inf": dict(d=(INF, 3.0)), "d<0": dict(d=(3.0, -2.0)),
}
PAIR_AT_FAULTS = {"mol_a=NULL": dict(mol_a=None), "mol_b=NULL": dict(mol_b=None), "mol_a=nan": dict(mol_a=NAN),
                  "mol_b=inf": dict(mol_b=INF)}

# two arguments wrong at once: the earlier check of today's order must go on winning
SOLUTE_DOUBLES = [
    ("sig=NULL", "charge=nan"), ("charge=NULL", "eps<0"), ("temperature=0", "eps=nan"), ("temperature=nan", "eps=inf"),
    ("n_sites=17", "charge=NULL"), ("n_insert=0", "charge=inf"), ("boltz_sum=NULL", "sig<0"), ("eps<0", "sig<0"),
    ("charge=nan", "eps=nan"), ("eps=inf", "sig=nan"),
]
PAIR_DOUBLES = [
    ("sig_a=NULL", "charge_a=nan"), ("charge_b=NULL", "eps_a<0"), ("temperature=0", "eps_a=nan"),
    ("temperature=nan", "eps_b=inf"), ("sig_b=NULL", "charge_a=inf"), ("eps_ab=NULL", "sig_a<0"),
    ("charge_b=nan", "sig_a<0"), ("eps_b<0", "eps_ab=nan"), ("n_sites=15+2", "charge_a=NULL"), ("n_sep=0", "eps_a=NULL"),
    ("n_insert=0", "sig_b=nan"), ("sig_ab<0", "eps_a=inf"),
]


def _rows():
    """{row id: (call helper, its keywords)}, ids 'entry point:fault[+fault]'."""
    rows = {}

    def add(entry, helper, fixed, faults, doubles=()):
        for name, kw in faults.items():
            rows[f"{entry}:{name}"] = (helper, {**fixed, **kw})
        for first, second in doubles:
            rows[f"{entry}:{first}+{second}"] = (helper, {**fixed, **faults[first], **faults[second]})

    for at in (False, True):
        own = MOL_FAULTS if at else OFFSETS_FAULTS
        second = next(iter(own))
        add("mmc_batch_widom_at" if at else "mmc_batch_widom", widom_call, dict(at=at), {**INSERT_FAULTS, **own},
            [("temperature=0", second), ("n_insert=0", second)])
        add("mmc_batch_widom_solute_at" if at else "mmc_batch_widom_solute", solute_call, dict(at=at),
            {**SOLUTE_FAULTS, **INSERT_FAULTS, **own}, SOLUTE_DOUBLES + [("sig<0", list(own)[1]), (second, "charge=nan")])
        own = PAIR_AT_FAULTS if at else PAIR_DRAWN_FAULTS
        add("mmc_batch_widom_pair_at" if at else "mmc_batch_widom_pair", pair_call, dict(at=at), {**PAIR_FAULTS, **own},
            PAIR_DOUBLES + [(next(iter(own)), "charge_b=nan"), ("sig_b<0", list(own)[2])])
    add("mmc_batch_set_solute", set_solute_call, {}, {**SOLUTE_FAULTS, **MOL_FAULTS},
        [d for d in SOLUTE_DOUBLES if not set(d) & set(INSERT_FAULTS)] + [("mol=NULL", "charge=nan"), ("sig<0", "mol=nan")])
    add("mmc_batch_deletion", deletion_call, {}, {"temperature=0": dict(temperature=0.0),
                                                  "temperature=nan": dict(temperature=NAN)})
    return rows


ROWS = _rows()


def _result(row):
    helper, kw = ROWS[row]
    st, msg = helper(**kw)
    return [int(st), msg]


def _recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_and_the_recorded_file_hold_the_same_rows():
    assert sorted(_recorded()) == sorted(ROWS)


@pytest.mark.parametrize("row", sorted(ROWS))
def test_a_refusal_keeps_its_status_text_and_place(row):
    got = _result(row)
    assert got[0] != _lib.MMC_OK
    assert got == _recorded()[row]


def test_the_library_reproduces_the_recorded_file_byte_for_byte():
    with open(GOLDEN) as f:
        assert f.read() == _dump()


def _dump():
    return json.dumps({row: _result(row) for row in sorted(ROWS)}, indent=1) + "\n"


if __name__ == "__main__":
    import sys
    if "--record" in sys.argv:
        with open(GOLDEN, "w") as f:
            f.write(_dump())
        print(f"{len(ROWS)} rows -> {GOLDEN}")
