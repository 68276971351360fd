"""Host front end: the reference's LP text -> SimplexMatrix -> the device engine.

A clean-room restatement of the reference's front end
for callers that do not link the reference CLI (integration/ does that): the
same input format, the same standard form and the same SimplexMatrix, quirks
included, so that ``build_smatrix(text)`` equals what the reference's
``CreateSMatrix`` builds from the same file (tests/test_frontend.py pins it to
the reference binary's transcripts). Stages, each citing what it restates:

* ``parse``        Parser / WriteIn / FormulaParser / FormulaSimplify
                   (Source/dataReader.c:148-235, 444-498, 301-386, 395-432),
                   numbers through Fractionize (basicFuncs.c:165-291)
* ``lp_trans``     LPTrans (dataReader.c:45-140), CmbSmlTerms (basicFuncs.c:338-366)
* ``standardize``  LPStandardize (simplex.c:91-230), CreateSlack / TermsSort /
                   VarCmp / InvertNegVars (simplex.c:269-354)
* ``align``        LPAlign (simplex.c:238-260)
* ``smatrix``      CreateSMatrix (matrix.c:19-91) -- the lack list written
                   correctly (the reference writes it through ``*lack[p++]`` and
                   crashes on two or more lacking rows, matrix.c:86)
* ``solve``        the device solve and readout the bridge performs
                   (integration/lpg_bridge.c LPGSolveSMatrix): rows without a
                   true unit column get artificials (two-phase or Big-M)
* ``solve_ilp``    integer LPs (the reference's wish-list, README): branch and
                   bound whose node LPs are a batch, a level per
                   BatchEngine.branch + solve_dual ("Branching"),
                   optionally after rounds of Gomory cuts at the root
                   (BatchEngine.cut, DESIGN.md §3.7, "Cuts")
* ``solve_scenarios``  models that differ only in their right-hand sides: the
                   first solved, the others restated from its tableau on the
                   device and re-optimised by the dual simplex
                   (BatchEngine.scenario, DESIGN.md §3.7, "Scenarios")
* ``solve_binary``  0-1 programs by implicit enumeration (the reference's
                   wish-list, README), one BinaryBatch per shape; and
                   ``solve_binary_text`` for the reference's model text with
                   every variable 0-1 ("0-1 programs")

The variable table mirrors hashTable.c (PutVarItem replaces an existing key in
place; GetVarItems walks buckets in hash order, VarHash hashTable.c:148-167).
Numbers follow the reference's ``long`` arithmetic step for step (RNum:
Fractionize, FractionAdd / NAdd, NInv, GCD / LCM with their wrap-around
overflow checks, numOprts.c / basicFuncs.c), so exactly the models whose
arithmetic the reference rejects are rejected; the SimplexMatrix is then
handed on as exact rationals.
The symbolic constant M is refused: user input may not carry it
(dataReader.c:413-417).

Nothing here computes on the host what the engine computes: the pivots run in
liblpg (``Engine``); this module only turns text into the tableau and the
engine's column 0 back into variable values.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from fractions import Fraction
from math import gcd

import numpy as np

_I64 = 1 << 63


class FrontendError(ValueError):
    """The reference would mark the model invalid (or crash) here."""


# ---- the reference's `long` arithmetic, operation for operation -------------
# Every coefficient of the reference is a pair of C longs, and its sums and
# products are guarded by checks that rely on wrap-around (numOprts.c:19-26,
# 37-129; basicFuncs.c:123-158; the reference is built -O0 -fwrapv). RNum
# redoes each step with explicit 64-bit wrap, so a value the reference's
# checks reject (an intermediate that wraps, though the reduced result would
# fit) is rejected here too, and an invalid value keeps the numerator and
# denominator the reference keeps (a later sum may use them). Where the
# reference's own arithmetic traps (x / 0, LONG_MIN / -1: SIGFPE on x86-64)
# the model is refused instead (tests/test_frontend.py records these).
# host/lpfront.c carries the same restatement in C.
_I64MIN, _I64MAX = -_I64, _I64 - 1


def _w64(x: int) -> int:
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= _I64 else x


def _cdiv(a: int, b: int) -> int:
    """C division (truncating); the trapping cases of x86-64 idiv refuse the model."""
    if b == 0 or (a == _I64MIN and b == -1):
        raise FrontendError("ERROR: arithmetic trap (the reference dies with SIGFPE here)")
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _cmod(a: int, b: int) -> int:
    return a - b * _cdiv(a, b)


def _labs(a: int) -> int:
    return _w64(-a) if a < 0 else a               # labs(LONG_MIN) == LONG_MIN


def _rgcd(a: int, b: int) -> int:
    """GCD, basicFuncs.c:123-137."""
    a, b = _labs(a), _labs(b)
    if b > a:
        a, b = b, a
    while b:
        a, b = b, _cmod(a, b)
    return a


def _rlcm(a: int, b: int) -> int:
    """LCM, basicFuncs.c:145-158: -1 when the product wraps."""
    d = _rgcd(a, b)
    a, b = _labs(a), _labs(b)
    q = _cdiv(a, d)
    r = _w64(q * b)
    if q != 0 and _cdiv(r, q) != b:
        return -1
    return r


def _d2l(x: float) -> int:
    """(long) of a double as x86-64 converts it: out of range or NaN -> LONG_MIN."""
    if not (-9223372036854775808.0 <= x < 9223372036854775808.0):
        return _I64MIN
    return int(x)


def _w32(x: int) -> int:
    x &= (1 << 32) - 1
    return x - (1 << 32) if x >= 1 << 31 else x


def _d2i(x: float) -> int:
    """(int) of a double as x86-64 converts it: out of range or NaN -> INT_MIN."""
    if not (-2147483648.0 <= x < 2147483648.0):
        return -(1 << 31)
    return int(x)


class RNum:
    """A reference Number without a constant: (numerator, denominator, valid)."""
    __slots__ = ("num", "den", "valid")

    def __init__(self, num: int, den: int, valid: bool = True):
        self.num, self.den, self.valid = num, den, valid

    def __neg__(self):                            # NInv, numOprts.c:290-294: no check
        return RNum(_w64(-self.num), self.den, self.valid)

    def __add__(self, o):                         # NAdd -> FractionAdd, numOprts.c:77-196
        pn, pd, nn, nd = self.num, self.den, o.num, o.den
        if pd == 0 or nd == 0:
            return RNum(0, 0, False)
        valid = True
        cm = _rlcm(pd, nd)
        if cm == -1:
            valid = False
        pf = _cdiv(cm, pd)
        pa = _w64(pn * pf)
        nf = _cdiv(cm, nd)
        na = _w64(nn * nf)
        if (pn != 0 and _cdiv(pa, pn) != pf) or (nn != 0 and _cdiv(na, nn) != nf):
            valid = False
        if (pa > 0 and na > _I64MAX - pa) or (pa < 0 and na < _I64MIN - pa):   # OFAdd
            return RNum(0, 0, False)
        s, den = pa + na, cm
        g = _rgcd(s, den)
        return RNum(_cdiv(s, g), _cdiv(den, g), valid)

    def mul_m1(self):
        """NMul(Fractionize("-1"), x) = FractionMul(-1, 1, n, d) (numOprts.c:37-66; the
        free-variable split, simplex.c:131, 154): its check divides -n by -1, which
        traps for n = LONG_MIN."""
        if self.den == 0:
            return RNum(0, 0, False)
        p = _w64(-self.num)
        _cdiv(p, -1)
        return RNum(p, self.den)

    def value(self) -> Fraction:
        return Fraction(self.num, self.den)

    def __repr__(self):
        return f"RNum({self.num}/{self.den}{'' if self.valid else ' invalid'})"


def _strtol(s: str):
    """C strtol(s, &end, 10): (value, fully consumed)."""
    i, n = 0, len(s)
    while i < n and s[i] in " \t\n\v\f\r":
        i += 1
    j = i
    if j < n and s[j] in "+-":
        j += 1
    k = j
    while k < n and s[k] in "0123456789":
        k += 1
    if k == j:
        return 0, n == 0
    v = int(s[i:k])
    return max(-_I64, min(_I64 - 1, v)), k == n


def _tokens(s: str, d: str):
    return [t for t in s.split(d) if t]          # strtok: empty tokens skipped


def fractionize(s: str) -> RNum:
    """Fractionize (basicFuncs.c:165-291) without constants."""
    bad = RNum(0, 0, False)
    if "M" in s:
        raise FrontendError("Simplification Failed: Manual added CONSTANTs are not allowed.")
    if "/" in s:
        tk = _tokens(s, "/")
        if not tk:
            return bad
        num, ok = _strtol(tk[0])
        if not ok or len(tk) < 2:
            return bad
        den, ok2 = _strtol(tk[1])
        if not ok2 or num == 0:
            return bad
        g = _labs(_rgcd(num, den))
        den = _cdiv(den, g)
        num = _cdiv(num, g)
        return RNum(num, den, den > 0)            # basicFuncs.c:219-220: a denominator <= 0 is invalid
    if s == "" or s in ("+", "-"):
        s = s + "1"
    if "." in s:
        try:
            dec = float(s)
        except ValueError:
            return bad
        tk = _tokens(s, ".")
        if len(tk) < 2:
            return bad
        den = _d2l(10.0 ** len(tk[1]))
        num = _d2l(dec * float(den))              # (long)(decimal * denominator): truncation (basicFuncs.c:264)
        g = _labs(_rgcd(num, den))
        return RNum(_cdiv(num, g), _cdiv(den, g))  # no denominator check on this path (basicFuncs.c:262-270)
    v, ok = _strtol(s)
    return RNum(v, 1) if ok else bad


def _dec(x) -> float:
    """Decimalize (basicFuncs.c:298-313): (double) n / d; 0 for an invalid number or d = 0.
    Takes an RNum, or a Fraction of the SimplexMatrix handed on."""
    if isinstance(x, Fraction):
        return float(x.numerator) / float(x.denominator)
    return float(x.num) / float(x.den) if (x is not None and x.valid and x.den) else 0.0


@dataclass
class Term:
    coef: object                 # RNum (the reference's Number, valid or not)
    var: str = ""
    inverted: bool = False

    def copy(self):
        return Term(self.coef, self.var, self.inverted)


@dataclass
class Formula:
    left: list = field(default_factory=list)
    right: list = field(default_factory=list)
    relation: int = 0            # -2 <=, -1 <, 1 >, 2 >=, 3 =


@dataclass
class VarItem:
    name: str
    relation: int                # 0 unrestricted, +-2 sign constraint / slack
    number: int = 0
    former: str = ""             # x = former - latter for an unrestricted x
    latter: str = ""


def _valid_var(s: str) -> bool:
    """ValidVar (basicFuncs.c:374-377): a letter, then digits only."""
    return len(s) > 0 and s[0].isascii() and s[0].isalpha() and all(c in "0123456789" for c in s[1:])


def _var_hash(s: str) -> int:
    """VarHash (hashTable.c:148-167); 0 = not storable."""
    if not s or not _valid_var(s):
        return 0
    h = ord(s[0]) + sum(ord(ch) - 48 for ch in s[1:]) - 65
    return h if h > 0 else 0


class VarTable:
    """The reference's variable hash table (hashTable.c)."""

    def __init__(self):
        self.items: dict = {}    # name -> VarItem, in insertion order (replacement keeps the slot)
        self.max_x = 0

    def put(self, item: VarItem) -> bool:
        h = _var_hash(item.name)
        if not h:
            return False
        sub, _ = _strtol(item.name[1:])
        if item.name[0] == "x" and sub > self.max_x:
            self.max_x = sub
        self.items[item.name] = item
        return True

    def get(self, name: str):
        return self.items.get(name) if _var_hash(name) else None

    def ordered(self):
        """GetVarItems order: by bucket (hash), then chain (insertion) order."""
        return sorted(self.items.values(), key=lambda it: _var_hash(it.name))


@dataclass
class Model:
    otype: int = 0               # 1 max, -1 min
    zcoef: object = None
    objective: list = field(default_factory=list)   # right-hand terms of the objective
    rows: list = field(default_factory=list)        # Formula per constraint
    vars: VarTable = field(default_factory=VarTable)


def _formula(s: str) -> Formula:
    """FormulaParser + FormulaSimplify (dataReader.c:301-432)."""
    f = Formula()
    side = 0
    cfc = False
    coef = None
    buf = ""
    i, n = 0, len(s)
    while i < n + 1:
        ch = s[i] if i < n else "+"
        if ch in "+->=<":
            if buf or (coef is not None and coef.valid):
                t = Term(coef if coef is not None else RNum(0, 0, False))
                if not buf and coef is not None and coef.valid:
                    t.var = ""
                elif all(c in "0123456789/+-.M" for c in buf):   # IsConstTerm
                    t.coef, t.var = fractionize(buf), ""
                else:
                    t.var = buf[:3]
                    if not _valid_var(t.var):
                        raise FrontendError(f"ERROR: Invalid variable name: {t.var}")
                cfc = False
                (f.left if side == 0 else f.right).append(t)
                buf, coef = "", None
            if ch in "+-":
                buf += ch
            elif ch in "<>":
                mark = -1 if ch == "<" else 1
                if i + 1 < n and s[i + 1] == "=":
                    mark *= 2
                    i += 1
                f.relation, side = mark, 1
            else:
                f.relation, side = 3, 1
        else:
            if not cfc and ch not in "0123456789./":
                coef = fractionize(buf) if buf else RNum(1, 1)
                buf, cfc = "", True
            buf += ch
        i += 1
    if not f.left or not f.right or not f.relation:
        raise FrontendError("Simplification Failed: Formula invalid.")
    # FormulaSimplify: the common divisors of every numerator and every
    # denominator, valid or not, from the first term's own values; each one
    # divided in place (C division, no reduction)
    joined = f.left + f.right
    gn, gd = joined[0].coef.num, joined[0].coef.den
    for t in joined[1:]:
        gn, gd = _rgcd(gn, t.coef.num), _rgcd(gd, t.coef.den)
    for t in joined:
        t.coef = RNum(_cdiv(t.coef.num, gn), _cdiv(t.coef.den, gd), t.coef.valid)
    return f


def parse(text: str) -> Model:
    """Parser (dataReader.c:148-235) with WriteIn (dataReader.c:444-498)."""
    if isinstance(text, bytes):
        text = text.decode("utf-8", "surrogateescape")
    m = Model()
    flag = 0
    bracket = False
    buf = ""
    have_of = False
    for ch in text + "\0":                         # the trailing char stands for the EOF step
        if ch == "{":
            stop, bracket = True, True
        elif ch == "}":
            stop, bracket = True, False
        else:
            stop = (not bracket and ch in " \t\n\v\f\r") or ch == ";"
        if not stop:
            if ch in " \t\n\v\f\r" or ch == "\0":
                continue
            buf += ch
        elif buf:
            if buf == "OF":
                flag = 1
            elif buf == "ST":
                flag = 2
            elif flag == 1:
                sp = buf.split(":")
                if len(sp) < 2 or sp[0] not in ("max", "min"):
                    raise FrontendError("Objective function invalid.")
                if have_of:
                    raise FrontendError("There can be only ONE Objective function!")
                f = _formula(sp[1])
                if f.relation != 3:
                    raise FrontendError("Wrong relational operator in Objective function!")
                if len(f.left) != 1 or _dec(f.left[0].coef) != 1:
                    raise FrontendError("Non-standard Objective function!")
                m.otype = 1 if sp[0] == "max" else -1
                m.zcoef = f.left[0].coef
                m.objective = f.right
                have_of = True
            elif flag == 2:
                m.rows.append(_formula(buf))
            buf = ""
        if ch == "}":
            flag = 0
    if not have_of:
        raise FrontendError("MISSING DATA: Objective Function not found.")
    if not m.rows:
        raise FrontendError("MISSING DATA: Constraints not found.")
    return m


def _combine(terms: list, table: VarTable, record: bool) -> None:
    """CmbSmlTerms (basicFuncs.c:338-366); record: register the variables (constraints)."""
    j = 0
    while j < len(terms):
        k = j + 1
        while k < len(terms):
            if terms[j].var == terms[k].var:
                terms[j].coef = terms[j].coef + terms[k].coef
                del terms[k]
                k -= 1
            k += 1
        if not terms[j].coef.valid:
            raise FrontendError("CMB ERROR: Invalid coefficient appeared after combining.")
        if terms[j].coef.num == 0:
            del terms[j]
            j -= 1
        elif record:
            table.put(VarItem(terms[j].var, 0))
        j += 1


def lp_trans(m: Model) -> Model:
    """LPTrans (dataReader.c:45-140): constants right, variables left, like terms
    combined, sign constraints x >= 0 / x <= 0 moved into the variable table."""
    _combine(m.objective, m.vars, record=False)
    i = 0
    while i < len(m.rows):
        st = m.rows[i]
        j = 0
        while j < len(st.left):                    # j advances past the shifted term (the reference's loop)
            if st.left[j].var == "":
                t = st.left.pop(j)
                t.coef = -t.coef
                st.right.append(t)
            j += 1
        j = 0
        while j < len(st.right):
            if st.right[j].var != "":
                t = st.right.pop(j)
                t.coef = -t.coef
                st.left.append(t)
            j += 1
        if not st.left or not st.right:
            raise FrontendError(f"ERROR: LPModel invalid due to the incomplete CONSTRAINT (ST Line: {i + 1}).")
        _combine(st.left, m.vars, record=True)
        for j in range(len(st.right) - 1, 0, -1):
            st.right[0].coef = st.right[0].coef + st.right[j].coef
            del st.right[j]
        if not st.left:
            raise FrontendError(f"ERROR: No term left in the left hand side of the CONSTRAINT (ST Line: {i + 1}) "
                                "after combining similar terms.")
        if not st.right[0].coef.valid:
            raise FrontendError(f"ERROR: Division by zero appeared in the right hand side of the CONSTRAINT "
                                f"(ST Line: {i + 1}).")
        if (len(st.left) == 1 and len(st.right) == 1 and _dec(st.left[0].coef) == 1
                and _dec(st.right[0].coef) == 0 and abs(st.relation) == 2):
            m.vars.put(VarItem(st.left[0].var, st.relation))
            del m.rows[i]
            continue
        i += 1
    nof = sum(1 for t in m.objective if t.var)
    if len(m.vars.items) != nof:
        raise FrontendError("ERROR: Mismatch in the number of variables in the Objective Function and Constraints.")
    return m


def _varcmp(a: str, b: str) -> int:
    """VarCmp (simplex.c:316-325)."""
    ca, cb = (a[:1] or "\0"), (b[:1] or "\0")
    if ca != cb:
        return 1 if ca > cb else -1
    sa = _strtol(a[1:])[0] if len(a) > 1 else 0
    sb = _strtol(b[1:])[0] if len(b) > 1 else 0
    return sa - sb


def _sort(terms: list) -> None:
    """TermsSort (simplex.c:288-305): selection sort, swaps as the reference's."""
    for i in range(len(terms)):
        mi = i
        for j in range(i + 1, len(terms)):
            if _varcmp(terms[mi].var, terms[j].var) > 0:
                mi = j
        if mi != i:
            terms[i], terms[mi] = terms[mi], terms[i]


def _invert_neg(terms: list, table: VarTable) -> None:
    """InvertNegVars (simplex.c:343-354): x <= 0 becomes x' = -x >= 0."""
    for t in terms:
        it = table.get(t.var)
        if it is not None and it.relation < 0 and it.number == 0:
            t.coef = -t.coef
            t.inverted = True


def standardize(m: Model, dual: bool = False) -> Model:
    """LPStandardize (simplex.c:91-230). Primal form (dual = 0): rows with a
    negative right-hand side are negated. Dual form (dual = 1, simplex.c:178-179):
    every > / >= row is negated into < / <= instead, whatever the sign of b, so
    each inequality gets a +1 slack (the dual simplex's starting basis; the
    reference's router never reaches this branch, router.c:32-34)."""
    sub = [m.vars.max_x]

    def slack():
        sub[0] += 1
        name = f"x{sub[0]}"
        m.vars.put(VarItem(name, 2))
        return Term(RNum(0, 1), name)

    if m.otype != 1:
        m.otype = 1
        m.zcoef = -m.zcoef
        for t in m.objective:
            t.coef = -t.coef
    i = 0
    while i < len(m.objective):
        t = m.objective[i]
        it = m.vars.get(t.var)
        if it is not None and it.relation == 0:    # unrestricted: x = x'' - x'
            target, c = t.var, t.coef
            former = slack()
            former.coef = c
            m.objective[i] = former
            latter = slack()
            latter.coef = c.mul_m1()
            m.objective.insert(i + 1, latter)
            it.former, it.latter = former.var, latter.var
            i += 1
            for st in m.rows:
                k = 0
                while k < len(st.left):
                    if st.left[k].var == target:
                        ck = st.left[k].coef
                        st.left[k] = Term(ck, former.var, former.inverted)
                        st.left.insert(k + 1, Term(ck.mul_m1(), latter.var, latter.inverted))
                        k += 1
                    k += 1
        i += 1
    for st in m.rows:
        b = st.right[0]
        if (not dual and _dec(b.coef) < 0) or (dual and st.relation > 0 and st.relation != 3):
            b.coef = -b.coef
            for t in st.left:
                t.coef = -t.coef
            if st.relation != 3:
                st.relation = -st.relation
        if st.relation != 3:
            s = slack()
            m.objective.append(s)
            s = s.copy()
            s.coef = RNum(-1, 1) if st.relation > 0 else RNum(1, 1)
            st.relation = 3
            st.left.append(s)
        _sort(st.left)
        _invert_neg(st.left, m.vars)
    _sort(m.objective)
    _invert_neg(m.objective, m.vars)
    return m


def align(m: Model) -> Model:
    """LPAlign (simplex.c:238-260): every row lists the objective's variables, 0 where absent."""
    for st in m.rows:
        k = 0
        for t in m.objective:
            if t.var:
                if k >= len(st.left) or st.left[k].var != t.var:
                    z = t.copy()
                    z.coef = RNum(0, 1)
                    st.left.insert(k, z)
                k += 1
    return m


@dataclass
class SMatrix:
    """CreateSMatrix's SimplexMatrix (matrix.c:19-91) as exact rationals."""
    names: list                  # column variables 1..N (no prime)
    inverted: list               # x <= 0 columns (printed with a prime)
    costs: list                  # c_j (max form)
    rows: list                   # m x (N+1): b, a_i1 .. a_iN
    basis: list                  # 1-based basic column per row, 0 = lacking (the identity heuristic)
    lacking: list
    constant: Fraction           # the objective constant CreateSMatrix drops
    zcoef: Fraction              # -1 when the model was a min
    vars: VarTable = None

    @property
    def display_names(self):
        return [v + ("'" if inv else "") for v, inv in zip(self.names, self.inverted)]


def smatrix(m: Model) -> SMatrix:
    """CreateSMatrix (matrix.c:19-91), the lack list written correctly."""
    constant = sum((t.coef.value() for t in m.objective if not t.var), Fraction(0))
    of = [t for t in m.objective if t.var]
    rows = []
    for st in m.rows:
        if len(st.left) < len(of):
            raise FrontendError("ERROR occurred during the Standardization and the Alignment :( ")
        rows.append([st.right[0].coef] + [st.left[j].coef for j in range(len(of))])
    basis = [0] * len(rows)
    for j in range(len(of)):
        ident, pos = 0, 0
        for i, r in enumerate(rows):
            d = _dec(r[j + 1])
            if d == 1:
                pos = i
            ident = _w32(ident + (_d2i(d) if d >= 0 else 6))   # int identityPart, (int) decimalized
        if ident == 1:
            basis[pos] = j + 1
    rows = [[x.value() for x in r] for r in rows]
    return SMatrix([t.var for t in of], [t.inverted for t in of], [t.coef.value() for t in of], rows, basis,
                   [i for i, b in enumerate(basis) if b == 0], constant, m.zcoef.value(), m.vars)


def build_smatrix(text: str, dual: bool = False) -> SMatrix:
    """LP text -> the reference's SimplexMatrix (Parser, LPTrans, LPStandardize, LPAlign, CreateSMatrix);
    ``dual``: LPStandardize's dual form (for ``solve(method="dual")``)."""
    return smatrix(align(standardize(lp_trans(parse(text)), dual=dual)))


@dataclass
class LPSolution:
    status: str                  # OPTIMAL / UNBOUNDED / INFEASIBLE / ITER_LIMIT / NUMERIC
    pivots: int
    z: float = float("nan")      # the original objective (constant added, min sign restored)
    columns: dict = field(default_factory=dict)    # standard-form column -> value
    variables: dict = field(default_factory=dict)  # the user's variables, un-substituted
    method: str = "primal"


def engine_arrays(sm: SMatrix):
    """What solve() and solve_batch() hand to the engine for ``sm``:
    (rows [m, nc] float64, basis [m] int64, cost [nc] float64, nc0, nlack).
    Columns 0..nc0-1 are the SimplexMatrix's [b | a_1..a_N]; a row without a
    true unit basic column gets an artificial unit column (nc0 .., in row
    order: art_first = nc0, nlack of them, nc = nc0 + nlack); cost holds the
    max-form costs and zeros for the artificials (the engine's N = nc - 1
    entries and one unused trailing zero)."""
    m, nc0 = len(sm.rows), len(sm.names) + 1
    basis = list(sm.basis)
    for i in range(m):                              # keep a basic column only if it is a true unit column
        j = basis[i]
        if j and any(sm.rows[q][j] != (1 if q == i else 0) for q in range(m)):
            basis[i] = 0
    nlack = sum(1 for b in basis if b == 0)
    nc = nc0 + nlack
    rows = np.zeros((m, nc), dtype=np.float64)
    for i, r in enumerate(sm.rows):
        rows[i, :nc0] = [_dec(x) for x in r]
    a = nc0
    for i in range(m):
        if not basis[i]:
            rows[i, a] = 1.0
            basis[i] = a
            a += 1
    cost = np.zeros(nc, dtype=np.float64)
    cost[:nc0 - 1] = [_dec(c) for c in sm.costs]
    return rows, np.asarray(basis, dtype=np.int64), cost, nc0, nlack


def _readout(sm: SMatrix, sol: LPSolution, objective: float, xb, bas, nc: int) -> LPSolution:
    """The optimum's z, columns and un-substituted variables from x_B and the basis."""
    x = np.zeros(nc, dtype=np.float64)
    for i in range(len(bas)):
        x[bas[i] - 1] = xb[i]
    sol.z = (objective + _dec(sm.constant)) / _dec(sm.zcoef)
    sol.columns = {v: float(x[j]) for j, v in enumerate(sm.display_names)}
    val = {v: float(x[j]) for j, v in enumerate(sm.names)}
    for it in sm.vars.ordered():
        if it.relation == 0 and it.former:
            sol.variables[it.name] = val.get(it.former, 0.0) - val.get(it.latter, 0.0)
        elif it.relation < 0 and it.number == 0:
            sol.variables[it.name] = -val.get(it.name, 0.0)
        else:
            sol.variables[it.name] = val.get(it.name, 0.0)
    return sol


def batch_groups(sms) -> dict:
    """solve_batch's grouping: {(m, nc0, nlack): [input indices, ascending]}, keys in order of first appearance."""
    return _groups([engine_arrays(sm) for sm in sms])


def _groups(arrays) -> dict:
    groups = {}
    for idx, (rows, _, _, nc0, nlack) in enumerate(arrays):
        groups.setdefault((rows.shape[0], nc0, nlack), []).append(idx)
    return groups


def solve_batch(sms, rule=None, device: int = 0, *, method: str = "two_phase", ragged: bool = False) -> list:
    """solve(sm, method=method) for every SMatrix of ``sms``, the models of one
    shape (m, nc0, nlack) together in one BatchEngine: one launch per group
    instead of one engine per model. ``method`` as solve()'s: "two_phase" or
    "big_m" where rows lack a basic column (the plain primal simplex where none
    does), or "dual" (every model must pass solve()'s two checks: no row without
    a slack basis, no positive max-form cost; the FrontendError names the first
    offending model and no device work has started). Unlike solve(), which takes
    an unknown method for "two_phase", any other method is a FrontendError: a
    misspelt method would otherwise cost a whole batch. The result list is in
    input order and each entry equals solve(sm, method=method) field by field,
    floats bit for bit. ``ragged=True`` gives the same results from at most two
    ragged batches whatever the shapes: one for the models the plain primal or
    the dual simplex solves, one for those that need artificials."""
    from . import _lib as L
    from .engine import BatchEngine
    if method not in ("two_phase", "big_m", "dual"):
        raise FrontendError(f"solve_batch: unknown method {method!r}")
    if rule is None:
        rule = L.RULE_DANTZIG
    sms = list(sms)
    arrays = [engine_arrays(sm) for sm in sms]
    if method == "dual":
        for idx, sm in enumerate(sms):
            if arrays[idx][4]:
                raise FrontendError(f"dual simplex: model {idx} has rows without a slack basis (equality rows); use "
                                    "build_smatrix(text, dual=True)")
            if any(_dec(c) > 0 for c in sm.costs):
                raise FrontendError(f"dual simplex: the slack basis of model {idx} is not dual feasible (a positive "
                                    "max-form cost)")
    out = [None] * len(sms)
    if ragged:
        plain = [idx for idx, a in enumerate(arrays) if method == "dual" or a[4] == 0]
        lacking = [idx for idx, a in enumerate(arrays) if method != "dual" and a[4] > 0]
        for members, art in ((plain, False), (lacking, True)):
            if not members:
                continue
            bigm = art and method == "big_m"
            tabs = []
            for idx in members:
                m, nc = arrays[idx][0].shape
                T = np.zeros((m + (2 if bigm else 1), nc), dtype=np.float64)
                T[:m] = arrays[idx][0]
                tabs.append(T)
            costs = [arrays[idx][2][:-1] for idx in members]
            with BatchEngine.ragged([arrays[idx][0].shape for idx in members], device=device, big_m=bigm) as e:
                e.load(tabs, [arrays[idx][1] for idx in members])
                if not art:
                    e.set_objective(costs)
                    res, used = (e.solve_dual(), "dual") if method == "dual" else (e.solve(rule=rule), "primal")
                elif bigm:
                    res, used = e.solve_big_m([arrays[idx][3] for idx in members], costs, rule=rule), "big_m"
                else:
                    res, used = e.solve_two_phase([arrays[idx][3] for idx in members], costs, rule=rule), "two_phase"
                rows, bas = e.get_rows(), e.get_basis()
            for q, idx in enumerate(members):
                r, m = res[q], arrays[idx][0].shape[0]
                sol = LPSolution(r.status_name, int(r.pivots), method=used)
                if r.status == L.OPTIMAL:
                    _readout(sms[idx], sol, r.objective, rows[q][:m, 0], bas[q], arrays[idx][0].shape[1])
                out[idx] = sol
        return out
    for (m, nc0, nlack), members in _groups(arrays).items():
        nc = nc0 + nlack
        bigm = method == "big_m" and nlack > 0
        T = np.zeros((len(members), m + (2 if bigm else 1), nc), dtype=np.float64)
        for q, idx in enumerate(members):
            T[q, :m] = arrays[idx][0]
        basis = np.array([arrays[idx][1] for idx in members], dtype=np.int64)
        cost = np.array([arrays[idx][2] for idx in members], dtype=np.float64)
        with BatchEngine(len(members), m, nc, device=device, big_m=bigm) as e:
            e.load(T, basis)
            if method == "dual":
                e.set_objective(cost)
                res, used = e.solve_dual(), "dual"
            elif nlack == 0:
                e.set_objective(cost)
                res, used = e.solve(rule=rule), "primal"
            elif bigm:
                res, used = e.solve_big_m(nc0, cost, rule=rule), "big_m"
            else:
                res, used = e.solve_two_phase(nc0, cost, rule=rule), "two_phase"
            rows, bas = e.get_rows(), e.get_basis()
        for q, idx in enumerate(members):
            r = res[q]
            sol = LPSolution(r.status_name, int(r.pivots), method=used)
            if r.status == L.OPTIMAL:
                _readout(sms[idx], sol, r.objective, rows[q, :m, 0], bas[q], nc)
            out[idx] = sol
    return out


@dataclass
class GoalModel:
    """A preemptive goal programme over n variables x >= 0 (include/lpg.h, "goal programmes").
    Hard rows: A x (sense) b with sense -1 (<=), 0 (=) or +1 (>=). Goal rows: G x + d- - d+ = target with
    d-, d+ >= 0. ``under[i]`` / ``over[i]``: None, or (level, weight > 0): the weight of goal i's
    under-achievement d- / over-achievement d+ in the sum that priority level ``level`` (1 the highest)
    minimises."""
    A: object
    sense: object
    b: object
    G: object
    target: object
    under: list
    over: list


@dataclass
class GoalSolution:
    """solve_goal's result for one model."""
    status: str                  # OPTIMAL / UNBOUNDED / INFEASIBLE / ITER_LIMIT / NUMERIC
    x: np.ndarray                # [n]; NaN unless OPTIMAL, like under, over and attained
    under: np.ndarray            # d- of every goal
    over: np.ndarray             # d+ of every goal
    attained: np.ndarray         # [L]: the weighted deviation that user level 1..L ends with
    pivots: int


def goal_arrays(model: GoalModel, idx: int = 0):
    """What solve_goal hands to a goal batch for ``model``: (rows [m, ncols] float64, basis [m] int64,
    costs [K, ncols - 1] float64, nart, L). Rows: the hard rows, then the goal rows; a row with a negative
    right-hand side is multiplied by -1 (a hard row's sense turns, a goal row's d- and d+ swap signs).
    Columns: [b | x_1..x_n | d-_1 d+_1 .. d-_g d+_g | a slack (<=) or surplus (>=) per hard row that has
    one, in row order | an artificial per hard = or >= row, in row order]. Basis: the slack, the
    artificial, or the deviation column that holds +1. With artificials K = L + 1 and device level 0 is
    theirs (cost -1 each), user level l being device level l; without, K = L and user level l is device
    level l - 1. A minimised deviation is the negative cost -weight at its level."""
    from . import _lib as L_
    A, G = np.atleast_2d(np.asarray(model.A, dtype=np.float64)), np.atleast_2d(np.asarray(model.G, dtype=np.float64))
    b, t = np.asarray(model.b, dtype=np.float64).reshape(-1), np.asarray(model.target, dtype=np.float64).reshape(-1)
    sense = np.asarray(model.sense, dtype=np.int64).reshape(-1)
    nh, ng = b.shape[0], t.shape[0]
    if A.size == 0:
        A = np.zeros((0, G.shape[1]))
    n = G.shape[1]
    if ng < 1 or n < 1 or A.shape != (nh, n) or G.shape != (ng, n) or sense.shape != (nh,):
        raise FrontendError(f"solve_goal: model {idx} has shapes A {A.shape}, sense {sense.shape}, b {b.shape}, G {G.shape}, "
                            f"target {t.shape}; want [h, n], [h], [h], [g, n], [g] with g >= 1")
    if not all(np.isfinite(a).all() for a in (A, b, G, t)) or not np.isin(sense, (-1, 0, 1)).all():
        raise FrontendError(f"solve_goal: model {idx} has an entry that is not finite, or a sense other than -1, 0, +1")
    if len(model.under) != ng or len(model.over) != ng:
        raise FrontendError(f"solve_goal: model {idx} has {ng} goals but {len(model.under)} / {len(model.over)} priorities")
    top = 0
    for pr in list(model.under) + list(model.over):
        if pr is None:
            continue
        level, weight = pr
        if int(level) != level or level < 1 or not (weight > 0) or not np.isfinite(weight):
            raise FrontendError(f"solve_goal: model {idx} has the priority {pr!r}; want (level >= 1, weight > 0)")
        top = max(top, int(level))
    if top < 1:
        raise FrontendError(f"solve_goal: model {idx} minimises no deviation")
    if top + 1 > L_.GOAL_MAX_LEVELS:
        raise FrontendError(f"solve_goal: model {idx} has {top} priority levels; with the level of the artificials "
                            f"that is more than the {L_.GOAL_MAX_LEVELS} a goal batch prices")
    flip = b < 0
    A, b, sense = np.where(flip[:, None], -A, A), np.where(flip, -b, b), np.where(flip, -sense, sense)
    nslack, nart = int((sense != 0).sum()), int((sense >= 0).sum())
    m, ncols = nh + ng, 1 + n + 2 * ng + nslack + nart
    K, shift = (top + 1, 0) if nart else (top, 1)
    rows, basis, costs = np.zeros((m, ncols)), np.zeros(m, dtype=np.int64), np.zeros((K, ncols - 1))
    s, a = 1 + n + 2 * ng, 1 + n + 2 * ng + nslack
    for i in range(nh):
        rows[i, 0], rows[i, 1:1 + n] = b[i], A[i]
        if sense[i] != 0:
            rows[i, s] = -float(sense[i])
            if sense[i] < 0:
                basis[i] = s
            s += 1
        if sense[i] >= 0:
            rows[i, a], basis[i], costs[0, a - 1] = 1.0, a, -1.0
            a += 1
    for i in range(ng):
        r, dm, dp = nh + i, 1 + n + 2 * i, 2 + n + 2 * i
        sign = -1.0 if t[i] < 0 else 1.0
        rows[r, 0], rows[r, 1:1 + n] = sign * t[i], sign * G[i]
        rows[r, dm], rows[r, dp] = sign, -sign
        basis[r] = dm if sign > 0 else dp
        for col, pr in ((dm, model.under[i]), (dp, model.over[i])):
            if pr is not None:
                costs[int(pr[0]) - shift, col - 1] = -float(pr[1])
    return rows, basis, costs, nart, top


def solve_goal(models, rule=None, device: int = 0, max_pivots: int = None) -> list:
    """The preemptive goal programme of every GoalModel of ``models``: the models of one (m, ncols, K)
    together in one goal batch (goal_arrays says what is loaded), one launch per group, the results in
    input order. A model whose hard rows need artificials is INFEASIBLE where their level ends below
    -1e-9 max(1, sum_i |T[i][0]|), Big-M's test. ``max_pivots``: 50 (m + ncols) by default."""
    from . import _lib as L
    from .engine import BatchEngine
    if rule is None:
        rule = L.RULE_DANTZIG
    arrays = [goal_arrays(mod, idx) for idx, mod in enumerate(models)]
    groups = {}
    for idx, (rows, _, costs, _, _) in enumerate(arrays):
        groups.setdefault((rows.shape[0], rows.shape[1], costs.shape[0]), []).append(idx)
    out = [None] * len(arrays)
    for (m, ncols, K), members in groups.items():
        T = np.zeros((len(members), m + K, ncols))
        for q, idx in enumerate(members):
            T[q, :m] = arrays[idx][0]
        with BatchEngine(len(members), m, ncols, device=device, levels=K) as e:
            e.load(T, np.array([arrays[idx][1] for idx in members], dtype=np.int64))
            res, attain = e.solve_goal(np.array([arrays[idx][2] for idx in members]),
                                       50 * (m + ncols) if max_pivots is None else max_pivots, rule)
            rows, bas = e.get_rows(), e.get_basis()
        for q, idx in enumerate(members):
            out[idx] = _goal_readout(models[idx], arrays[idx], res[q].status, int(res[q].pivots), attain[q], rows[q, :m, 0],
                                     bas[q])
    return out


def _goal_readout(model, arrays, status, pivots, attain, xb, bas) -> GoalSolution:
    """GoalSolution of one model from its status, attained device levels, x_B and basis."""
    from . import _lib as L
    _, _, costs, nart, top = arrays
    ng = len(model.under)
    n = np.atleast_2d(np.asarray(model.G)).shape[1]
    if nart and status in (L.OPTIMAL, L.UNBOUNDED):
        bsum = 0.0
        for v in xb:                                   # in row order, as the Big-M kernels add it
            bsum += abs(float(v))
        if attain[0] < -1e-9 * (bsum if bsum > 1.0 else 1.0):
            status = L.INFEASIBLE
    nan = float("nan")
    sol = GoalSolution(L.STATUS_NAMES[status], np.full(n, nan), np.full(ng, nan), np.full(ng, nan), np.full(top, nan), pivots)
    if status == L.OPTIMAL:
        val = np.zeros(costs.shape[1] + 1)
        for i in range(len(bas)):
            val[bas[i]] = xb[i]
        sol.x = val[1:1 + n].copy()
        sol.under, sol.over = val[1 + n:1 + n + 2 * ng:2].copy(), val[2 + n:2 + n + 2 * ng:2].copy()
        sol.attained = -np.asarray(attain[1 if nart else 0:], dtype=np.float64)
    return sol


@dataclass
class AssignmentSolution:
    """solve_assignment's result for one cost matrix, in the caller's orientation."""
    status: str                  # OPTIMAL / INFEASIBLE
    objective: float             # NaN if infeasible
    assignment: np.ndarray       # the column of every row; -1 for a row left out (more rows than columns) or infeasible
    u: np.ndarray                # the row potentials [rows]
    v: np.ndarray                # the column potentials [columns]
    steps: int


def solve_assignment(costs, maximize: bool = False, device: int = 0) -> list:
    """The assignment problem of every 2-D cost matrix of ``costs`` (include/lpg.h,
    "assignment"): the matrices of one shape together in one AssignmentBatch, one
    launch per shape, the results in input order. min(rows, columns) pairs are
    chosen, no row and no column twice, with the smallest (``maximize``: largest)
    cost sum; +inf forbids a pair. A matrix with more rows than columns is solved
    transposed and reported back in the caller's orientation: ``assignment`` is
    still the column per row (-1 for the rows left out), u belongs to the rows
    and v to the columns."""
    from . import _lib as L
    from .engine import AssignmentBatch
    mats = []
    for idx, c in enumerate(costs):
        c = np.asarray(c, dtype=np.float64)
        if c.ndim != 2 or c.shape[0] < 1 or c.shape[1] < 1:
            raise FrontendError(f"solve_assignment: matrix {idx} has shape {c.shape}, want 2-D and not empty")
        mats.append(c)
    groups = {}
    for idx, c in enumerate(mats):
        tr = c.shape[0] > c.shape[1]
        groups.setdefault((min(c.shape), max(c.shape)), []).append((idx, tr))
    out = [None] * len(mats)
    for (nr, nc), members in groups.items():
        stack = np.stack([mats[idx].T if tr else mats[idx] for idx, tr in members])
        with AssignmentBatch(len(members), nr, nc, device=device, maximize=maximize) as a:
            a.load(stack)
            res = a.solve()
            col, u, v = a.get()
        for q, (idx, tr) in enumerate(members):
            r = res[q]
            if tr:
                # the batch's rows are the caller's columns: invert col, swap the potentials
                asg = np.full(nc, -1, dtype=np.int64)
                if r.status == L.OPTIMAL:
                    asg[col[q]] = np.arange(nr)
                pu, pv = v[q].copy(), u[q].copy()
            else:
                asg, pu, pv = col[q].copy(), u[q].copy(), v[q].copy()
            out[idx] = AssignmentSolution(L.STATUS_NAMES[r.status], float(r.objective), asg, pu, pv, int(r.steps))
    return out


@dataclass
class TransportSolution:
    """solve_transportation's result for one model, the dummy row or column stripped."""
    status: str                  # OPTIMAL, ITER_LIMIT, or INFEASIBLE (the optimum ships over a forbidden route)
    objective: float             # NaN if infeasible
    x: np.ndarray                # the flows [sources, sinks]
    u: np.ndarray                # the source potentials
    v: np.ndarray                # the sink potentials
    iterations: int
    unused: np.ndarray           # per source: supply that stays (total supply above total demand), else zeros
    unmet: np.ndarray            # per sink: demand that is not served (total demand above total supply), else zeros


def solve_transportation(models, maximize: bool = False, start: str = "least_cost", rule: int = 0, max_iters: int = None,
                         device: int = 0) -> list:
    """The transportation problem of every (costs, supply, demand) of ``models``
    (include/lpg.h, "transportation"): the models of one shape together in one
    TransportBatch, the results in input order. Data are integers. An
    unbalanced model gets a zero-cost dummy column (supply left over) or dummy
    row (demand not served), which is stripped from the answer and reported as
    ``unused`` / ``unmet``. A cost of +inf (``maximize``: -inf) forbids a route:
    it is replaced by a penalty M = (cmax - cmin) T + |cmin| + 1 on the
    minimised costs, T the total amount, which any plan that ships one unit over
    such a route pays above every plan that ships none; the model is INFEASIBLE
    if the optimum still uses one. A penalty outside the library's caps is an
    error."""
    from . import _lib as L
    from .engine import TransportBatch
    prepared = []
    for idx, (c, s, d) in enumerate(models):
        c, s, d = np.asarray(c, dtype=np.float64), np.asarray(s, dtype=np.float64), np.asarray(d, dtype=np.float64)
        if c.ndim != 2 or c.shape[0] < 1 or c.shape[1] < 1 or s.shape != (c.shape[0],) or d.shape != (c.shape[1],):
            raise FrontendError(f"solve_transportation: model {idx} has shapes {c.shape}, {s.shape}, {d.shape}, want "
                                f"[nr, nc], [nr], [nc]")
        if not (np.isfinite(s).all() and np.isfinite(d).all()) or (s < 0).any() or (d < 0).any():
            raise FrontendError(f"solve_transportation: model {idx} has a supply or demand that is negative or not finite")
        nr, nc = c.shape
        cost = -c if maximize else c.copy()                # minimised
        forbidden = cost == np.inf
        if np.isnan(cost).any() or (cost == -np.inf).any():
            raise FrontendError(f"solve_transportation: model {idx} has a NaN cost or an infinity of the wrong sign")
        diff = s.sum() - d.sum()
        if diff > 0:                                       # a dummy sink takes what stays
            cost, forbidden = np.hstack([cost, np.zeros((nr, 1))]), np.hstack([forbidden, np.zeros((nr, 1), dtype=bool)])
            d = np.append(d, diff)
        elif diff < 0:                                     # a dummy source serves what is missing
            cost, forbidden = np.vstack([cost, np.zeros((1, nc))]), np.vstack([forbidden, np.zeros((1, nc), dtype=bool)])
            s = np.append(s, -diff)
        if forbidden.any():
            finite = cost[~forbidden]
            cmax, cmin = (finite.max(), finite.min()) if finite.size else (0.0, 0.0)
            total = s.sum()
            big = (cmax - cmin) * total + abs(cmin) + 1.0
            if big > L.TRANSPORT_COST_CAP or big * total > 2.0 ** 53:
                raise FrontendError(f"solve_transportation: model {idx}: the penalty {big:g} of a forbidden route at a "
                                    f"total amount of {total:g} is outside the caps (2^40, and 2^53 for the product)")
            cost = np.where(forbidden, big, cost)
        prepared.append((-cost if maximize else cost, s, d, forbidden, nr, nc, diff))
    groups = {}
    for idx, p in enumerate(prepared):
        groups.setdefault(p[0].shape, []).append(idx)
    out = [None] * len(prepared)
    for (gr, gc), members in groups.items():
        with TransportBatch(len(members), gr, gc, maximize=maximize, start=start, device=device) as t:
            t.load(np.stack([prepared[i][0] for i in members]), np.stack([prepared[i][1] for i in members]),
                   np.stack([prepared[i][2] for i in members]))
            res = t.solve(max_iters, rule)
            x, u, v, _ = t.get()
        for q, idx in enumerate(members):
            _, _, _, forbidden, nr, nc, diff = prepared[idx]
            r = res[q]
            status, objective = L.STATUS_NAMES[r.status], float(r.objective)
            if r.status == L.OPTIMAL and (x[q][forbidden] > 0).any():
                status, objective = "INFEASIBLE", float("nan")
            out[idx] = TransportSolution(status, objective, x[q, :nr, :nc].copy(), u[q, :nr].copy(), v[q, :nc].copy(),
                                         int(r.iterations), x[q, :nr, nc].copy() if diff > 0 else np.zeros(nr),
                                         x[q, nr, :nc].copy() if diff < 0 else np.zeros(nc))
    return out


@dataclass
class BinarySolution:
    """solve_binary's result for one 0-1 program, in the caller's column order."""
    status: str                  # OPTIMAL, INFEASIBLE, or ITER_LIMIT (max_nodes reached: the incumbent so far)
    objective: float             # NaN when no point was found
    x: np.ndarray                # int8 0 / 1; -1 throughout when no point was found
    nodes: int
    names: list = None           # solve_binary_text: the variable of every entry of x


def binary_order(c, order) -> np.ndarray:
    """The columns in the order the device is given them: "cost": by descending |c_j|, ties to the smaller j (the
    textbook's ordering: the bound bites early); None: as given."""
    c = np.asarray(c, dtype=np.float64)
    if order is None:
        return np.arange(len(c))
    if order != "cost":
        raise FrontendError(f"solve_binary: order {order!r} unknown (\"cost\" or None)")
    return np.array(sorted(range(len(c)), key=lambda j: (-abs(c[j]), j)), dtype=np.int64)


def binary_split(count: int, m: int, n: int, maximize: bool = False, device: int = 0) -> int:
    """The smallest split that gives a batch of `count` problems at least as many waves as the device holds at
    once (BinaryBatch.resident_waves: the occupancy query for the instantiation that split selects)."""
    from . import _lib as L
    from .engine import BinaryBatch
    top = min(n, L.BINARY_MAX_SPLIT)
    for s in range(top + 1):
        with BinaryBatch(count, m, n, split=s, maximize=maximize, device=device) as b:
            if (count << s) >= b.resident_waves:
                return s
    return top


def _binary_batch(A, sense, rhs, c, maximize, split, max_nodes, device):
    """One batch of one shape on the device: (status, found, nodes, objective) per problem and x [count, n]."""
    from .engine import BinaryBatch
    count, m, n = A.shape
    if split is None:
        split = binary_split(count, m, n, maximize, device)
    with BinaryBatch(count, m, n, split=split, maximize=maximize, device=device) as b:
        b.load(A, sense, rhs, c)
        res = b.solve(max_nodes)
        return [(r.status, r.found, r.nodes, r.objective) for r in res], b.get()


def solve_binary(models, maximize: bool = False, split=None, order="cost", max_nodes: int = 0, device: int = 0) -> list:
    """The 0-1 program of every (A, sense, rhs, c) of ``models`` (include/lpg.h, "0-1 programs"): minimise
    (``maximize``: maximise) c.x subject to a_i.x {<=, =, >=} b_i (sense -1, 0, +1), x binary, on integer data.
    The models of one shape run together in one BinaryBatch; the results come back in input order, x in the
    caller's column order whatever ``order`` presents to the device."""
    from . import _lib as L
    items = []
    for idx, mod in enumerate(models):
        if len(mod) != 4:
            raise FrontendError(f"solve_binary: model {idx} is not a tuple (A, sense, rhs, c)")
        A, sense, rhs, c = (np.asarray(a) for a in mod)
        if A.ndim != 2 or A.shape[0] < 1 or A.shape[1] < 1 or sense.shape != (A.shape[0],) or rhs.shape != (A.shape[0],) \
                or c.shape != (A.shape[1],):
            raise FrontendError(f"solve_binary: model {idx} has shapes {A.shape}, {sense.shape}, {rhs.shape}, {c.shape}, "
                                "want [m, n], [m], [m], [n]")
        perm = binary_order(c, order)
        items.append((np.asarray(A, dtype=np.float64)[:, perm], sense.astype(np.int32), rhs.astype(np.float64),
                      np.asarray(c, dtype=np.float64)[perm], perm))
    groups = {}
    for idx, it in enumerate(items):
        groups.setdefault(it[0].shape, []).append(idx)
    out = [None] * len(items)
    for (m, n), members in groups.items():
        stack = [np.stack([items[idx][f] for idx in members]) for f in range(4)]
        res, x = _binary_batch(stack[0], stack[1], stack[2], stack[3], maximize, split, max_nodes, device)
        for q, idx in enumerate(members):
            xo = np.full(n, -1, dtype=np.int8)
            xo[items[idx][4]] = x[q]
            out[idx] = BinarySolution(L.STATUS_NAMES[res[q][0]], float(res[q][3]), xo, int(res[q][2]))
    return out


def binary_model(text: str):
    """The reference's model text as a 0-1 program on integers: (A, sense, rhs, c, maximize, names, scale,
    offset). Every variable is binary: a sign-constraint line x >= 0 is accepted and ignored, x <= 0 refused.
    Each row and the objective are scaled to integers by the least common multiple of their denominators
    (`scale`: the objective's; the model's own objective is c.x / scale + offset). A strict < or > on the
    integer row becomes <= b - 1 or >= b + 1."""
    from functools import cmp_to_key
    m = lp_trans(parse(text))
    for it in m.vars.items.values():
        if it.relation < 0:
            raise FrontendError(f"solve_binary_text: {it.name} <= 0 contradicts a 0-1 variable")
    names = sorted(m.vars.items, key=cmp_to_key(_varcmp))
    col = {v: j for j, v in enumerate(names)}

    def lcm_of(values):
        d = 1
        for v in values:
            d = d * v.denominator // gcd(d, v.denominator)
        return d

    A = np.zeros((len(m.rows), len(names)))
    sense, rhs = np.zeros(len(m.rows), dtype=np.int32), np.zeros(len(m.rows))
    for i, st in enumerate(m.rows):
        coefs = [(t.var, t.coef.value()) for t in st.left]
        b = st.right[0].coef.value()
        d = lcm_of([v for _, v in coefs] + [b])
        for var, v in coefs:
            A[i, col[var]] = float(v * d)
        bi = int(b * d)
        if st.relation == 3:
            sense[i] = 0
        elif st.relation < 0:
            sense[i], bi = -1, (bi - 1 if st.relation == -1 else bi)
        else:
            sense[i], bi = 1, (bi + 1 if st.relation == 1 else bi)
        rhs[i] = float(bi)
    obj = [(t.var, t.coef.value()) for t in m.objective]
    scale = lcm_of([v for var, v in obj if var])
    c = np.zeros(len(names))
    offset = Fraction(0)
    for var, v in obj:
        if var:
            c[col[var]] = float(v * scale)
        else:
            offset += v
    return A, sense, rhs, c, m.otype == 1, names, scale, offset


def solve_binary_text(text: str, split=None, order="cost", max_nodes: int = 0, device: int = 0) -> BinarySolution:
    """The reference's model text with every variable 0-1 (binary_model), solved on the device; the objective is
    reported in the model's own scale."""
    A, sense, rhs, c, maximize, names, scale, offset = binary_model(text)
    sol = solve_binary([(A, sense, rhs, c)], maximize=maximize, split=split, order=order, max_nodes=max_nodes,
                       device=device)[0]
    if sol.objective == sol.objective:
        sol.objective = float(Fraction(int(sol.objective), scale) + offset)
    sol.names = names
    return sol


@dataclass
class LPSensitivity(LPSolution):
    """sensitivity_batch's result: the LPSolution and, for an OPTIMAL model, its sensitivity report."""
    basis: list = field(default_factory=list)        # the column basic in each standard-form row, by name
    shadow: list = field(default_factory=list)       # dz/db_i per standard-form row, in the user's objective sense
    rhs_range: list = field(default_factory=list)    # per row: (lowest b_i, highest b_i, (who leaves at each end))
    cost_range: dict = field(default_factory=dict)   # column -> (lowest c_j, highest c_j, (who enters at each end))


def _column_name(sm: SMatrix, j: int, nc0: int):
    """The name of engine column j (1-based): a standard-form column, or an artificial added for a lacking row."""
    return sm.display_names[j - 1] if j < nc0 else f"artificial{j - nc0 + 1}"


def sensitivity_batch(sms, rule=None, device: int = 0) -> list:
    """solve_batch(sms, rule) and the sensitivity report of every model, computed on the device from the solved
    tableaus (include/lpg.h, "ranging"): the same grouping by shape and the same methods (the plain primal
    simplex, or two-phase where rows lack a basic column), one ranging() call per group. Every entry is an
    LPSensitivity whose LPSolution fields equal solve_batch's bit for bit. For an OPTIMAL model, with ident =
    engine_arrays' basis (the unit column of every standard-form row):

    * ``basis[i]``: the column basic in row i at the optimum, by display name;
    * ``shadow[i]`` = (dual[i] + cost of column ident[i]) / zcoef: the change of ``z`` per unit of the
      standard-form right-hand side b_i, in the user's objective sense (a min model's sign restored, as ``z``);
    * ``rhs_range[i]`` = (b_i + lo, b_i + hi, (a, b)): the values of b_i between which the optimal basis stays
      feasible; a / b name the column basic in the row that limits the low / high end (the variable that leaves
      there), None where that end is infinite;
    * ``cost_range[name]`` = (c_j + lo, c_j + hi, (a, b)) for the standard-form columns: the values of the cost
      c_j between which the basis stays optimal, and the column that enters at each end or None. The costs are
      in MAX FORM, the ones SMatrix.costs holds: for a min model they are the negated user costs, and for a
      primed (x <= 0) column the cost of the substituted variable.

    The other models get the LPSolution fields alone."""
    from . import _lib as L
    from .engine import BatchEngine
    if rule is None:
        rule = L.RULE_DANTZIG
    sms = list(sms)
    arrays = [engine_arrays(sm) for sm in sms]
    out = [None] * len(sms)
    for (m, nc0, nlack), members in _groups(arrays).items():
        nc = nc0 + nlack
        T = np.zeros((len(members), m + 1, nc), dtype=np.float64)
        for q, idx in enumerate(members):
            T[q, :m] = arrays[idx][0]
        ident = np.array([arrays[idx][1] for idx in members], dtype=np.int64)
        cost = np.array([arrays[idx][2] for idx in members], dtype=np.float64)
        with BatchEngine(len(members), m, nc, device=device) as e:
            e.load(T, ident)
            if nlack == 0:
                e.set_objective(cost)
                res, used = e.solve(rule=rule), "primal"
            else:
                res, used = e.solve_two_phase(nc0, cost, rule=rule), "two_phase"
            rows, bas = e.get_rows(), e.get_basis()
            rg = e.ranging(ident)
        for q, idx in enumerate(members):
            r, sm = res[q], sms[idx]
            sol = LPSensitivity(r.status_name, int(r.pivots), method=used)
            out[idx] = sol
            if r.status != L.OPTIMAL:
                continue
            _readout(sm, sol, r.objective, rows[q, :m, 0], bas[q], nc)
            name = lambda j: _column_name(sm, int(j), nc0)
            zc, b, c = _dec(sm.zcoef), arrays[idx][0][:, 0], cost[q]
            sol.basis = [name(j) for j in bas[q]]
            sol.shadow = [float((rg.dual[q, i] + c[ident[q, i] - 1]) / zc) for i in range(m)]
            leaves = lambda r_: None if r_ < 0 else name(bas[q, r_])
            sol.rhs_range = [(float(b[i] + rg.rhs_lo[q, i]), float(b[i] + rg.rhs_hi[q, i]),
                              (leaves(rg.rhs_lo_at[q, i]), leaves(rg.rhs_hi_at[q, i]))) for i in range(m)]
            enters = lambda k: None if k < 1 else name(k)
            sol.cost_range = {name(j): (float(c[j - 1] + rg.cost_lo[q, j - 1]), float(c[j - 1] + rg.cost_hi[q, j - 1]),
                                        (enters(rg.cost_lo_at[q, j - 1]), enters(rg.cost_hi_at[q, j - 1])))
                              for j in range(1, nc0)}
    return out


def solve_scenarios(sms, rule=None, device: int = 0) -> list:
    """The optimum of every SMatrix of ``sms``, models that differ only in their right-hand sides (column 0 of
    the standard-form rows; engine_arrays' rows beyond column 0, basis, cost, nc0 and nlack must be equal, or a
    FrontendError names the first model that differs), warm-started on the device (include/lpg.h, "scenarios"):
    ``sms[0]`` is solved as solve() solves it (the primal simplex, or two-phase where rows lack a basic column) in
    a batch of one; scenario() makes one child per model, sms[0] included, from that solved tableau, the
    right-hand sides stated in the frame of the basis the model was loaded with; one solve_dual() re-optimises
    all of them. Every entry has ``method="scenario_dual"`` and the child's dual pivots as ``pivots``. Where the
    base is not OPTIMAL, or its final basis still holds an artificial column (the dual simplex would not keep
    that artificial at zero), or a column of the loaded basis has a cost (the restated objective would lack that
    cost times the right-hand side), the result is solve_batch(sms, rule)'s instead."""
    from . import _lib as L
    from .engine import BatchEngine
    if rule is None:
        rule = L.RULE_DANTZIG
    sms = list(sms)
    if not sms:
        return []
    arrays = [engine_arrays(sm) for sm in sms]
    rows, basis, cost, nc0, nlack = arrays[0]
    for idx, (r, b, c, n0, nl) in enumerate(arrays[1:], 1):
        if not (r.shape == rows.shape and (n0, nl) == (nc0, nlack) and np.array_equal(r[:, 1:], rows[:, 1:])
                and np.array_equal(b, basis) and np.array_equal(c, cost)):
            raise FrontendError(f"solve_scenarios: model {idx} differs from model 0 in more than its right-hand side")
    m, nc = rows.shape
    if cost[basis - 1].any():
        return solve_batch(sms, rule)
    T = np.zeros((1, m + 1, nc), dtype=np.float64)
    T[0, :m] = rows
    with BatchEngine(1, m, nc, device=device) as base:
        base.load(T, basis[None])
        if nlack:
            res = base.solve_two_phase(nc0, cost, rule=rule)
        else:
            base.set_objective(cost)
            res = base.solve(rule=rule)
        if res[0].status != L.OPTIMAL or (base.get_basis()[0] >= nc0).any():
            return solve_batch(sms, rule)
        with base.scenario(np.zeros(len(sms), dtype=np.int64), np.array([a[0][:, 0] for a in arrays]), basis) as e:
            res = e.solve_dual()
            tabs, bas = e.get_rows(), e.get_basis()
    out = []
    for q, sm in enumerate(sms):
        sol = LPSolution(res[q].status_name, int(res[q].pivots), method="scenario_dual")
        if res[q].status == L.OPTIMAL:
            _readout(sm, sol, res[q].objective, tabs[q, :m, 0], bas[q], nc)
        out.append(sol)
    return out


def solve(sm: SMatrix, method: str = "two_phase", rule=None, device: int = 0) -> LPSolution:
    """The bridge's device solve (integration/lpg_bridge.c LPGSolveSMatrix) on liblpg:
    rows without a true unit basic column get artificials (two-phase by default,
    ``method="big_m"`` for Big-M; ``method="dual"``: the dual simplex from the
    slack basis of a dual-form SimplexMatrix, which must be complete and dual
    feasible); the readout un-substitutes x <= 0 and free variables as the
    reference's variable table records them."""
    from . import _lib as L
    from .engine import Engine
    if rule is None:
        rule = L.RULE_DANTZIG
    rows, basis, cost, nc0, nlack = engine_arrays(sm)
    m, nc = rows.shape
    if method == "dual":
        if nlack:
            raise FrontendError("dual simplex: rows without a slack basis (equality rows); use build_smatrix(text, dual=True)")
        if any(_dec(c) > 0 for c in sm.costs):
            raise FrontendError("dual simplex: the slack basis is not dual feasible (a positive max-form cost)")
    bigm = method == "big_m" and nlack > 0
    with Engine(m, nc, device=device, flags=L.FLAG_BIG_M if bigm else 0) as e:
        e.load_rows(0, rows)
        e.set_basis(np.asarray(basis, dtype=np.int64))
        if method == "dual":
            e.set_objective(cost)
            r = e.solve_dual()
            used = "dual"
        elif nlack == 0:
            e.set_objective(cost)
            r = e.solve(rule=rule)
            used = "primal"
        elif bigm:
            r = e.solve_big_m(nc0, cost, rule=rule)
            used = "big_m"
        else:
            r = e.solve_two_phase(nc0, cost, rule=rule)
            used = "two_phase"
        sol = LPSolution(r.status_name, int(r.pivots), method=used)
        if r.status != L.OPTIMAL:
            return sol
        xb = e.get_column0()
        bas = e.get_basis()
    return _readout(sm, sol, r.objective, xb, bas, nc)


def solve_text(text: str, method: str = "two_phase", rule=None, device: int = 0) -> LPSolution:
    """LP text (the reference's input format) -> the optimum on the device."""
    return solve(build_smatrix(text, dual=method == "dual"), method=method, rule=rule, device=device)


@dataclass
class ILPSolution(LPSolution):
    """LPSolution of the best integer point found (status OPTIMAL, or NODE_LIMIT with the incumbent so far;
    INFEASIBLE when the tree holds none), `pivots` summed over every node LP."""
    nodes: int = 0               # node LPs solved: the root and every child made
    depth: int = 0               # levels of the tree that held an OPTIMAL node, the root's included


def text_variables(text: str) -> list:
    """The variables the text itself names (objective, then constraints, in order of appearance), from
    parse(text) before LPTrans moves sign constraints away and LPStandardize adds slacks."""
    m = parse(text)
    seen = []
    for t in m.objective + [t for st in m.rows for t in st.left + st.right]:
        if t.var and t.var not in seen:
            seen.append(t.var)
    return seen


def integer_mask(sm: SMatrix, integer) -> np.ndarray:
    """The uint8 mask over standard-form columns 1..len(sm.names) of the user's integer variables: a variable's
    own column (the inverted one of an x <= 0 variable), or both columns of a free variable x = former - latter
    (branching on whichever of the two is basic and fractional is complete: every integer x has a
    representation with one of them zero)."""
    mask = np.zeros(len(sm.names), dtype=np.uint8)
    for name in integer:
        it = sm.vars.get(name) if sm.vars is not None else None
        if it is None:
            raise FrontendError(f"solve_ilp: {name!r} is not a variable of the model")
        for col in ([it.former, it.latter] if (it.relation == 0 and it.former) else [name]):
            if col not in sm.names:
                raise FrontendError(f"solve_ilp: {name!r} has no column in the standard form")
            mask[sm.names.index(col)] = 1
    return mask


def solve_ilp(sm: SMatrix, integer, *, int_tol: float = 1e-6, node_limit: int = 100000, rule=None,
              device: int = 0, cut_rounds: int = 0, max_cuts: int = 8) -> ILPSolution:
    """Branch and bound on the device: the variables named in ``integer`` must be integers.

    Level-synchronous and breadth-first, fixed so that a CPU restatement follows it node for node
    (tests/branch_cases.py reference_walk; with cut rounds tests/cut_cases.py reference_walk). The root is solved
    as solve() solves it (the primal simplex, or two-phase where rows lack a basic column) in a batch of one.
    After an OPTIMAL root, up to ``cut_rounds`` rounds of Gomory mixed-integer cuts (include/lpg.h, "cuts"):
    cut_select lists the root's ``max_cuts`` most fractional rows (none: the rounds end); cut() makes the batch of
    one with those cuts and the parent is closed; solve_dual() re-optimises it, its pivots are added and it counts
    as one more node; an INFEASIBLE result ends the call as INFEASIBLE and any other status but OPTIMAL ends it
    with that status; the LP with its cuts is the root of the tree (depth 1). ``cut_rounds=0`` makes none of
    these calls. Then, per level: branch_select on the level's
    batch (``rule``: BRANCH_MOST_FRACTIONAL by default); of the nodes with no fractional integer variable the
    best (larger max-form objective, then lower index) replaces the incumbent if strictly better; a remaining
    node whose objective is <= the incumbent's is dropped; every survivor gets two children, down before up,
    parents ascending, all made by one branch() and re-optimised by one solve_dual(); INFEASIBLE children are
    dropped, OPTIMAL ones are the next level, any other status ends the call with it. The walk stops when a
    level is empty or more than ``node_limit`` node LPs have been solved (status NODE_LIMIT). The tableaus
    never leave the device: the host sees one status, objective and branching row per node, and the rows and
    basis of an incumbent."""
    from . import _lib as L
    from .engine import BatchEngine
    if rule is None:
        rule = L.BRANCH_MOST_FRACTIONAL
    mask = integer_mask(sm, integer)
    rows, basis, cost, nc0, nlack = engine_arrays(sm)
    m, nc = rows.shape
    T = np.zeros((1, m + 1, nc), dtype=np.float64)
    T[0, :m] = rows
    batch = BatchEngine(1, m, nc, device=device)
    try:
        batch.load(T, np.asarray(basis, dtype=np.int64)[None])
        if nlack:
            res, used = batch.solve_two_phase(nc0, cost), "two_phase"
        else:
            batch.set_objective(cost)
            res, used = batch.solve(), "primal"
        sol = ILPSolution(res[0].status_name, int(res[0].pivots), method=used, nodes=1, depth=1)
        if res[0].status != L.OPTIMAL:
            return sol
        for _ in range(cut_rounds):
            rows = batch.cut_select(mask, int_tol, max_cuts)[0]
            if not len(rows):
                break
            child = batch.cut([0], [rows], mask)
            batch.close()
            batch = child
            res = batch.solve_dual()
            sol.nodes += 1
            sol.pivots += int(res[0].pivots)
            if res[0].status != L.OPTIMAL:
                sol.status = res[0].status_name
                return sol
        alive, objective = [0], [res[0].objective]           # the level: LPs of `batch`, their objectives
        best = None                                          # (objective, x_B, basis, ncols) of the incumbent
        while alive:
            if sol.nodes > node_limit:
                sol.status = "NODE_LIMIT"
                break
            pick, _, _ = batch.branch_select(mask, int_tol, rule)
            cand = None
            for q in alive:
                if pick[q] < 0 and (cand is None or objective[q] > objective[cand]):
                    cand = q
            if cand is not None and (best is None or objective[cand] > best[0]):
                tab = batch.get_rows(cand, 1)[0]
                best = (objective[cand], tab[:-1, 0].copy(), batch.get_basis(cand, 1)[0], tab.shape[1])
            parents = [q for q in alive if pick[q] >= 0 and not (best is not None and objective[q] <= best[0])]
            if not parents:
                break
            src = np.repeat(np.asarray(parents, dtype=np.int64), 2)
            child = batch.branch(src, pick[src], np.tile(np.array([-1, 1], dtype=np.int8), len(parents)))
            batch.close()
            batch = child
            res = batch.solve_dual()
            sol.nodes += len(res)
            sol.pivots += sum(int(r.pivots) for r in res)
            other = [r for r in res if r.status not in (L.OPTIMAL, L.INFEASIBLE)]
            if other:
                sol.status = other[0].status_name
                return sol
            alive = [c for c, r in enumerate(res) if r.status == L.OPTIMAL]
            objective = [r.objective for r in res]
            if alive:
                sol.depth += 1
    finally:
        batch.close()
    if best is None:
        if sol.status == "OPTIMAL":
            sol.status = "INFEASIBLE"
        return sol
    return _readout(sm, sol, best[0], best[1], best[2], best[3])


def solve_ilp_text(text: str, integer=None, *, int_tol: float = 1e-6, node_limit: int = 100000, rule=None,
                   device: int = 0, cut_rounds: int = 0, max_cuts: int = 8) -> ILPSolution:
    """LP text -> the integer optimum; ``integer=None``: every variable the text itself names."""
    if integer is None:
        integer = text_variables(text)
    return solve_ilp(build_smatrix(text), integer, int_tol=int_tol, node_limit=node_limit, rule=rule, device=device,
                     cut_rounds=cut_rounds, max_cuts=max_cuts)


def main(argv=None) -> int:
    """``python -m linearprogramming_amd.frontend model.txt [--big-m] [--bland]``:
    the reference's input file solved on the device, non-interactively
    (many models that differ only in their right-hand sides: solve_scenarios)."""
    import argparse
    from . import _lib as L
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("path")
    ap.add_argument("--big-m", action="store_true", help="artificials by Big-M instead of two-phase")
    ap.add_argument("--dual", action="store_true", help="dual form and the dual simplex (dual-feasible models)")
    ap.add_argument("--bland", action="store_true", help="Bland's rule instead of Dantzig's")
    a = ap.parse_args(argv)
    method = "dual" if a.dual else ("big_m" if a.big_m else "two_phase")
    try:
        sm = build_smatrix(open(a.path, "rb").read(), dual=a.dual)
        sol = solve(sm, method=method, rule=L.RULE_BLAND if a.bland else L.RULE_DANTZIG)
    except FrontendError as ex:
        print(ex)
        return 2
    print(f"{sol.status} after {sol.pivots} pivots ({sol.method})")
    if sol.status == "OPTIMAL":
        print(f"\tz = {sol.z:.12g}")
        print("\t" + "".join(f"{k}={v:.12g} | " for k, v in sol.columns.items()))
        print("Variables:\n\t" + "".join(f"{k}={v:.12g} | " for k, v in sol.variables.items()))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
