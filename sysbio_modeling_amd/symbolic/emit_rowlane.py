"""Row-lane form of a model: SIMD across isomorphic equations.

The integrator kernels keep one trajectory per wavefront.  What is identical for all
sensitivity columns of a trajectory -- f(y), the non-zeros of J_y and of J_p -- is scalar work
per trajectory; evaluating it redundantly on all 64 lanes is what bounds the per-wave kernel
(rocprofv3: VALU-issue bound, ~40 % of the instructions).  Rate-law networks, however, are
made of a few kinetic forms repeated over many species: rows whose expression bundle
(f_i, dF_i/dy, dF_i/dp) is the same tree up to a renaming of symbols form a CLASS, and a class is
evaluated once, lane i working on row i with per-lane operands.  This module finds the classes
and prints

  * ``__constant__`` tables: class of each row, which state / parameter feeds each operand slot,
    where each produced J_y / J_p entry goes;
  * ``class_dispatch`` -- the class bodies, each run under the exec mask of its rows;
  * ``apply_rowlane`` -- dz_i = sum_m J_y[i,m] z_m + A[i][lane] for a sensitivity column, with
    J_y read (wave-uniform) and A read (one column per lane) from LDS: no per-lane selects.
"""
from __future__ import annotations

import re
from collections import OrderedDict

import sympy
from sympy import Symbol, cse


def _canonical(bundle, var_index, par_index):
    """Rename symbols to placeholders in order of first appearance (depth-first over the bundle).
    Returns (canonical expr tuple, [state indices per Y slot], [param indices per P slot])."""
    ys, ps = [], []
    mapping = {}
    for expr in bundle:
        for node in sympy.preorder_traversal(expr):
            if isinstance(node, Symbol) and node not in mapping:
                if node.name in var_index:
                    mapping[node] = Symbol('YS_%d' % len(ys))
                    ys.append(var_index[node.name])
                elif node.name in par_index:
                    mapping[node] = Symbol('PS_%d' % len(ps))
                    ps.append(par_index[node.name])
    canon = tuple(e.xreplace(mapping) for e in bundle)
    return canon, ys, ps


def find_classes(spec, d, align='derived'):
    """Group rows by the structure of (f_i, J_y entries of the row, J_p entries of the row).

    A class numbers its operands and outputs in order of first appearance, so two kinetic forms put the same role into
    different slots and ``class_dispatch`` selects between them for nothing.  ``align`` (default: what ``d`` chose,
    ``choose_alignment``) gives per class the POSITION of each of its state / parameter operands and J_y / J_p outputs:
    ``align[ci] = dict(ys=[...], ps=[...], jy=[...], jp=[...])``, entry k = the slot of the class's k-th operand or
    output in the first-appearance numbering.  Operand positions need not be dense: a class with fewer operands than
    another may leave any of their slots unused.  Output positions are a permutation of the class's own: the slot of
    an entry stays its index in d.jy_rows[i] / d.jp_rows[i].  None: the first-appearance numbering itself.

    Returns (classes, row_info).  A class: canon (f, the J_y entries, the J_p entries in the order of d.jy_base /
    d.jp_base -- the rows before alignment --, symbols YS_<slot> / PS_<slot>), rows, ys_slot / ps_slot / jy_slot /
    jp_slot.  A row: cls, ys / ps =
    state / parameter index per slot (None: a slot the row's class does not use)."""
    var_index = {v: i for i, v in enumerate(spec.variables)}
    par_index = {p: i for i, p in enumerate(spec.params)}
    classes = OrderedDict()   # key -> dict(canon, rows=[...])
    row_info = []
    jy_rows, jp_rows = getattr(d, 'jy_base', d.jy_rows), getattr(d, 'jp_base', d.jp_rows)
    for i in range(spec.n_vars):
        bundle = [d.f_c[i]] + [d.jy_c[e] for e, _ in jy_rows[i]] + [d.jp_c[e] for e, _ in jp_rows[i]]
        canon, ys, ps = _canonical(bundle, var_index, par_index)
        key = (sympy.srepr(canon), len(jy_rows[i]), len(jp_rows[i]))
        if key not in classes:
            classes[key] = dict(canon=canon, rows=[], n_jy=len(jy_rows[i]), n_jp=len(jp_rows[i]),
                                n_ys=len(ys), n_ps=len(ps))
        classes[key]['rows'].append(i)
        row_info.append(dict(cls=list(classes.keys()).index(key), ys=ys, ps=ps))
    classes = list(classes.values())
    if align == 'derived':
        align = getattr(d, 'align', None)
    _place(classes, align)
    if align is not None:
        for r in row_info:
            c = classes[r['cls']]
            for kind in ('ys', 'ps'):
                at = [None] * (max(c[kind + '_slot'] + [-1]) + 1)
                for k, s in enumerate(c[kind + '_slot']):
                    at[s] = r[kind][k]
                r[kind] = at
    return classes, row_info


def _place(classes, align):
    """give the classes (first-appearance numbering) the slot positions of ``align``"""
    for ci, c in enumerate(classes):
        a = align[ci] if align is not None else dict(ys=range(c['n_ys']), ps=range(c['n_ps']), jy=range(c['n_jy']),
                                                     jp=range(c['n_jp']))
        for kind in ('ys', 'ps', 'jy', 'jp'):
            c[kind + '_slot'] = list(a[kind])
            assert len(c[kind + '_slot']) == c['n_' + kind] == len(set(c[kind + '_slot']))
        if align is not None:
            rename = {Symbol('YS_%d' % k): Symbol('YS_%d' % s) for k, s in enumerate(c['ys_slot'])}
            rename.update({Symbol('PS_%d' % k): Symbol('PS_%d' % s) for k, s in enumerate(c['ps_slot'])})
            c['canon'] = tuple(e.xreplace(rename) for e in c['canon'])


def _n_slots(classes, kind):
    return max([s + 1 for c in classes for s in c[kind + '_slot']] + [1])


def emit_rowlane_tables(spec, d, printer_factory):
    """Namespace-scope ``__constant__`` tables + sizes; returns (lines, meta)."""
    classes, row_info = find_classes(spec, d)
    n = spec.n_vars
    max_ys, max_ps, max_jy, max_jp = (_n_slots(classes, kind) for kind in ('ys', 'ps', 'jy', 'jp'))
    tag = "SBM_RL"

    def table(name, rows_of_slots):
        flat = ", ".join(str(v) for slot in rows_of_slots for v in slot)
        return "__constant__ short %s_%s[%d] = {%s};" % (tag, name, len(rows_of_slots) * n, flat)

    def operand(i, kind, s):
        at = row_info[i][kind]
        return at[s] if s < len(at) and at[s] is not None else 0     # (an unused slot reads element 0: never used)

    ys_t = [[operand(i, 'ys', s) for i in range(n)] for s in range(max_ys)]
    ps_t = [[operand(i, 'ps', s) for i in range(n)] for s in range(max_ps)]
    nj = max(len(d.jy), 1)
    jy_t = [[(d.jy_rows[i][s][0] if s < len(d.jy_rows[i]) else nj) for i in range(n)] for s in range(max_jy)]
    # position in the additive matrix A[NV][64] (+ one spare slot at NV*64 for unused outputs)
    jp_t = [[(i * 64 + d.jp_rows[i][s][1] if s < len(d.jp_rows[i]) else n * 64) for i in range(n)] for s in range(max_jp)]
    # the column alone (-1: unused slot), for kernels that cut the columns into chunks (any number of columns)
    jpc_t = [[(d.jp_rows[i][s][1] if s < len(d.jp_rows[i]) else -1) for i in range(n)] for s in range(max_jp)]
    # the column of each J_y slot (-1: unused), for the kernel that hands J_y to the matrix cores as a dense tile
    jyc_t = [[(d.jy_rows[i][s][1] if s < len(d.jy_rows[i]) else -1) for i in range(n)] for s in range(max_jy)]
    L = ["// row-lane tables: [slot][row]",
         "__constant__ short %s_CLASS[%d] = {%s};" % (tag, n, ", ".join(str(r['cls']) for r in row_info)),
         table("YS", ys_t), table("PS", ps_t), table("JYOUT", jy_t), table("APOS", jp_t), table("JPCOL", jpc_t),
         table("JYCOL", jyc_t), ""]
    meta = dict(classes=classes, max_ys=max_ys, max_ps=max_ps, max_jy=max_jy, max_jp=max_jp,
                share_products=getattr(d, 'align', None) is not None)
    return L, meta


# Operations worth sharing between classes, in VALU issue slots of a wavefront (fp64 on gfx950: v_rcp_f64 and the other
# transcendentals issue at quarter rate; SBM_RCP adds two Newton steps of two FMAs).  A select is two v_cndmask_b32.
_OP_COST = {'rcp': 8, 'sqrt': 16, 'exp': 40, 'log': 40, 'pow': 80, 'call': 40, 'add': 1, 'mul': 1}
_SEL_COST = 2
_LEAF = re.compile(r'(?<![A-Za-z0-9_])(?:ys\[\d+\]|ps\[\d+\]|c\d+_x\d+|h\d+|t)(?![A-Za-z0-9_])')
_NAME = re.compile(r'(?<![A-Za-z0-9_])(?:c\d+_x\d+|h\d+)(?![A-Za-z0-9_])')


def _op_kind(node):
    """which entry of _OP_COST the root of ``node`` is (None: a leaf)"""
    if node.is_Function:
        return {'SBM_RCP': 'rcp', 'exp': 'exp', 'log': 'log'}.get(node.func.__name__, 'call')
    if node.is_Pow:
        if node.exp.is_Integer and 1 <= int(node.exp) <= 4:
            return 'mul'
        return 'sqrt' if node.exp == sympy.Rational(1, 2) else 'pow'
    if node.is_Add:
        return 'add'
    if node.is_Mul:
        return 'mul'
    return None


def _tree_cost(node):
    kind = _op_kind(node)
    if kind is None:
        return 0
    n = int(node.exp) - 1 if node.is_Pow and kind == 'mul' else max(len(node.args) - 1, 1)
    if node.is_Mul and node.args[0] == -1:
        n -= 1           # (a sign is a source modifier of the instruction that uses the product)
    return _OP_COST[kind] * n + sum(_tree_cost(a) for a in node.args)


def _plan_hoist(per_class, pr):
    """Operations that several classes have in common, to be evaluated ONCE on selected operands.

    Every class body is evaluated on every lane (class_dispatch below), so an operation that occurs in k classes costs k
    times what a lane needs.  Where the classes' subtrees under one root (reciprocal, sqrt, exp, log, pow; a sum or a
    product as well -- with the classes' slots aligned, choose_alignment, few of their operands differ)
    print to the SAME TEXT up to the operands at the leaves -- ys[.], ps[.], CSE temporaries, earlier shared values --
    the text is emitted once with each differing leaf replaced by a select chain on the class:
    op(sel(c, a, b)) and sel(c, op(a), op(b)) are the same value in every lane, and because the shared statement IS
    each class's own text after substitution of its leaves, operand order, association and what the compiler may
    contract into FMAs are those of the unshared form.  The class bodies are printed as before, with the subtree
    replaced by the shared name (``_ExprPrinter.shared``).

    Greedy, most expensive trees first; a group is taken when cost(tree) * (k - 1) exceeds the selects it adds,
    _SEL_COST per differing leaf and extra class.  Classes without the operation simply do not take part.
    Returns ([{node: name} per class], [dict(name, shape, leaves={class: [leaf texts]}, classes=[...])])."""
    n_cls = len(per_class)
    shared = [{} for _ in range(n_cls)]
    hoisted = []
    rejected = set()
    exprs = [[pr.normalised(e) for _, e in repl] + [pr.normalised(e) for e in red] for repl, red in per_class]
    temps = [[str(s) for s, _ in repl] for repl, _ in per_class]

    def depends(name, on, seen):
        """does statement ``name`` (a temporary or a shared value) use ``on``, directly or not"""
        if name in seen:
            return False
        seen.add(name)
        for ci in range(n_cls):
            if name in temps[ci]:
                pr.shared = shared[ci]
                uses = _NAME.findall(pr.doprint(exprs[ci][temps[ci].index(name)]))
                break
        else:
            h = next(h for h in hoisted if h['name'] == name)
            uses = [x for lv in h['leaves'].values() for x in lv if _NAME.fullmatch(x)]
        return any(u == on or depends(u, on, seen) for u in uses)

    def printed(ci, node):
        """text of ``node`` as class ci prints it, values shared so far by name; -> (shape, leaves)"""
        # a temporary that is a PRODUCT enters the shared text as its definition, not by name: where it feeds a sum the
        # compiler contracts the two into one FMA, which it could not do through a select of two finished products.
        # (Under a cheap root -- a sum, a product -- it stays a name: there the temporary IS the operand the classes
        # differ in, and the select of two finished values is what the sharing is for.)
        pr.shared = {k: v for k, v in shared[ci].items() if k != node}
        for (sym, _), e in zip(per_class[ci][0], exprs[ci]):
            if _op_kind(e) == 'mul' and _op_kind(node) not in ('add', 'mul'):
                pr.shared[sym] = "(%s)" % pr._print(e)
        text = pr._print(node)
        return _LEAF.sub('@', text), _LEAF.findall(text)

    def n_selects(leaves):
        """selects the operands cost: per leaf position, one for every class that differs from the most common operand"""
        return sum(len(pos) - max(pos.count(x) for x in pos) for pos in zip(*leaves))

    def cyclic(h):
        feeds = [x for lv in h['leaves'].values() for x in lv if _NAME.fullmatch(x)]
        return any(depends(x, h['name'], set()) for x in feeds)

    while True:
        groups = OrderedDict()     # (shape, occurrence) -> {class: (node, leaves)}
        for ci in range(n_cls):
            seen, count = set(), {}
            for e in exprs[ci]:
                walk = sympy.preorder_traversal(e)
                for node in walk:
                    if node in shared[ci]:
                        walk.skip()
                        continue
                    if node in seen or _op_kind(node) is None or _tree_cost(node) == 0:
                        continue
                    seen.add(node)
                    shape, leaves = printed(ci, node)
                    occ = count.get(shape, 0)
                    count[shape] = occ + 1
                    groups.setdefault((shape, occ), OrderedDict())[ci] = (node, leaves)
        best = None
        for key, members in groups.items():
            if len(members) < 2 or key in rejected:
                continue
            cost = _tree_cost(next(iter(members.values()))[0])
            gain = cost * (len(members) - 1) - _SEL_COST * n_selects([lv for _, lv in members.values()])
            if gain > 0 and (best is None or cost > best[0]):
                best = (cost, key, members)
        if best is None:
            break
        _, key, members = best
        name = 'h%d' % len(hoisted)
        h = dict(name=name, shape=key[0], classes=list(members), nodes={ci: nd for ci, (nd, _) in members.items()},
                 leaves={ci: lv for ci, (_, lv) in members.items()})
        hoisted.append(h)
        for ci, (node, _) in members.items():
            shared[ci][node] = name
        # a class's temporary that feeds the shared value must not itself need it (two classes with the same two
        # operations nested in opposite orders): such a group is left alone
        if cyclic(h):
            hoisted.pop()
            for ci, (node, _) in members.items():
                del shared[ci][node]
            rejected.add(key)
    # the larger trees were planned first: print them again, so that a smaller operation inside them that was shared
    # afterwards (it occurs elsewhere as well) is used by name there too
    for h in hoisted:
        again = {ci: printed(ci, h['nodes'][ci]) for ci in h['classes']}
        if len({shape for shape, _ in again.values()}) == 1:
            old = (h['shape'], h['leaves'])
            h['shape'], h['leaves'] = next(iter(again.values()))[0], {ci: lv for ci, (_, lv) in again.items()}
            if cyclic(h):
                h['shape'], h['leaves'] = old
    pr.shared = {}
    return shared, hoisted


def _sel_template(h):
    """the shared statement's right-hand side: the common text, each leaf the classes disagree on as a select chain whose
    default is the operand most of the participating classes have"""
    cls = h['classes']
    parts = h['shape'].split('@')
    out = [parts[0]]
    for pos in range(len(parts) - 1):
        col = [h['leaves'][ci][pos] for ci in cls]
        expr = max(col, key=lambda x: (col.count(x), len(col) - col[::-1].index(x)))
        default = expr
        for ci in reversed(cls):
            if h['leaves'][ci][pos] != default:
                expr = "SBM_SEL(is%d, %s, %s)" % (ci, h['leaves'][ci][pos], expr)
        out += [expr, parts[pos + 1]]
    return "".join(out)


def _share_products(repl, red, prefix):
    """A product that is a whole output of the class and also a group of factors of another output (a rate term
    y/(K + y) is d f / d Vmax, and f holds Vmax times it) is evaluated once, as a temporary: the other classes then meet
    ONE operand where this class has the product, and the sum around it can be shared (_plan_hoist)."""
    repl, red = list(repl), list(red)
    n_temp = len(repl)
    for e in list(red):
        if not (e.is_Mul and len(e.args) >= 2 and not e.args[0].is_Number):
            continue
        factors = set(e.args)

        def holds(m):
            return m.is_Mul and factors < set(m.args)
        if not any(x.has(e) or any(holds(m) for m in sympy.preorder_traversal(x)) for x in red if x != e):
            continue
        sym = Symbol('%s%d' % (prefix, n_temp))
        n_temp += 1
        repl.append((sym, e))
        red = [sym if x == e else x.replace(holds, lambda m: sympy.Mul(sym, *[a for a in m.args if a not in factors]))
               for x in red]
    return repl, red


_CALL = re.compile(r'(?<![A-Za-z0-9_])([A-Za-z_][A-Za-z0-9_]*)\(')


def _text_cost(lines):
    """static cost of printed statements on the scale of _OP_COST / _SEL_COST"""
    cost = 0
    for ln in lines:
        if '=' not in ln or ln.lstrip().startswith('//'):
            continue
        rhs = ln.split('=', 1)[1].split(';')[0]
        if rhs.lstrip().startswith('(cls =='):
            continue
        for name in _CALL.findall(rhs):
            cost += {'SBM_RCP': _OP_COST['rcp'], 'SBM_SEL': _SEL_COST, 'sqrt': _OP_COST['sqrt'], 'exp': _OP_COST['exp'],
                     'log': _OP_COST['log'], 'pow': _OP_COST['pow']}.get(name, _OP_COST['call'])
        cost += rhs.count('*') * _OP_COST['mul'] + (rhs.count(' + ') + rhs.count(' - ')) * _OP_COST['add']
    return cost


_MAX_CANDIDATES = 600     # all combinations up to here ...
_MAX_GREEDY = 300         # ... beyond it, this many two-class bodies


def choose_alignment(spec, d, make_printer):
    """Slot positions per class (the ``align`` of find_classes) that make ``class_dispatch`` cheapest, or None when no
    choice beats the first-appearance numbering (ties go to it: such a model prints as it always did).

    The class with the most slots keeps its numbering.  For every other class the candidates are the placements of its
    state operands and of its parameter operands among the slots of the widest class of each kind (a class with fewer
    may leave any of them unused) and the permutations of its J_y outputs and of its J_p outputs.  Each candidate is
    PRINTED -- with the sharing of _plan_hoist, whatever ``class_hoist`` the caller prints with, and with
    _share_products -- and costed by _text_cost.  All combinations of all classes when there are at most
    _MAX_CANDIDATES of them.  Otherwise greedy, one pass: each class against the reference class alone (a two-class
    body prints in milliseconds whatever the number of classes) -- all combinations of the class where they are few,
    because roles move together (the saturating state, its rate constant and the entry they make), else one slot kind
    at a time -- until _MAX_GREEDY bodies have been printed.  Candidates are enumerated in lexicographic order and only
    a strictly lower cost replaces the incumbent: deterministic."""
    import math
    from itertools import islice, permutations, product, repeat
    base, _ = find_classes(spec, d, align=None)
    if len(base) < 2:
        return None
    kinds = ('ys', 'ps', 'jy', 'jp')
    width = {k: max(c['n_' + k] for c in base) for k in kinds}
    n_slots = {k: max(width[k], 1) for k in kinds}
    ref = max(range(len(base)), key=lambda ci: (sum(base[ci]['n_' + k] for k in kinds), -ci))
    others = [ci for ci in range(len(base)) if ci != ref]
    identity = [{k: tuple(range(c['n_' + k])) for k in kinds} for c in base]
    memo = {}            # (the CSE of a class depends on its operand positions alone)

    def cost(align, only=None):
        classes = [dict(c) for c in base]
        _place(classes, align)
        if only is not None:
            classes = [classes[ci] for ci in sorted(only)]
        return _text_cost(_dispatch_body(classes, n_slots, make_printer, hoist=True, share_products=True, memo=memo))

    # (candidates are counted arithmetically and taken lazily: a row with n entries has n! orders of them)
    def placements(ci, k):
        n_own = base[ci]['n_' + k]
        return permutations(range(width[k] if k in ('ys', 'ps') else n_own), n_own)

    def n_placements(ci, k):
        n_own = base[ci]['n_' + k]
        return math.perm(width[k] if k in ('ys', 'ps') else n_own, n_own)

    def combos(ci):
        return (dict(zip(kinds, combo)) for combo in product(*[placements(ci, k) for k in kinds]))

    def n_combos(ci):
        return math.prod(n_placements(ci, k) for k in kinds)

    _place(base, None)
    plain = _text_cost(_dispatch_body(base, n_slots, make_printer, hoist=True, share_products=False))
    n_all = 1
    for ci in others:
        n_all = min(n_all * n_combos(ci), _MAX_CANDIDATES + 1)
    if n_all <= _MAX_CANDIDATES:
        best, best_cost = identity, cost(identity)
        for choice in product(*[combos(ci) for ci in others]):
            cand = list(identity)
            for ci, a in zip(others, choice):
                cand[ci] = a
            c = cost(cand) if cand != identity else best_cost
            if c < best_cost:
                best, best_cost = cand, c
        return best if best_cost < plain else None
    best = list(identity)
    for ci in others:
        pair_cost = cost(best, only=(ref, ci))
        if n_combos(ci) <= _MAX_GREEDY // 4:
            rounds = [combos(ci)]
        else:
            rounds = [zip(repeat(k), placements(ci, k)) for k in kinds]
        share = max(_MAX_GREEDY // (len(others) * len(rounds)), 1)       # (of the budget, for this round of this class)
        for trials in rounds:
            for a in islice(trials, share):
                if isinstance(a, tuple):                  # (one kind moves, the others stay where the class has them)
                    a = dict(best[ci], **{a[0]: a[1]})
                if a == best[ci]:
                    continue
                c = cost(best[:ci] + [a] + best[ci + 1:], only=(ref, ci))
                if c < pair_cost:
                    best[ci], pair_cost = a, c
    return best if cost(best) < plain else None


def _class_cse(ci, canon, share_products):
    """(temporaries, outputs) of class ``ci`` as ``class_dispatch`` prints them"""
    repl, red = cse(list(canon), symbols=sympy.numbered_symbols('c%d_x' % ci), optimizations='basic')
    if share_products:
        repl, red = _share_products(repl, red, 'c%d_x' % ci)
    return repl, red


class _NotZero(Exception):
    pass


def _f_at_zero_operands(repl, f):
    """Value of a class's ``f`` (with the temporaries ``repl`` it is printed with) when every state and parameter
    operand is 0, found by walking the expression bottom-up in exact arithmetic.  Raises _NotZero where the walk cannot
    vouch for the floating-point result: a node that is not finite (a reciprocal or logarithm of 0, 0/0), a dependence on
    ``t``, or a sum with more than one non-zero term (zero would then rest on a cancellation that rounding may miss).
    What is left is exact in floating point too: a product with a zero factor and finite others is 0, a sum of zeros
    and at most one other term is that term."""
    temps = {sym: e for sym, e in repl}
    seen = {}

    def value(node):
        if node in seen:
            return seen[node]
        if isinstance(node, Symbol):
            if node in temps:
                v = value(temps[node])
            elif node.name.startswith(('YS_', 'PS_')):
                v = sympy.S.Zero
            else:
                raise _NotZero(node)
        elif node.is_Atom:
            v = node
        else:
            args = [value(a) for a in node.args]
            if node.is_Add and sum(1 for a in args if a != 0) > 1:
                raise _NotZero(node)
            if getattr(node.func, '__name__', '') == 'SBM_RCP':      # (emit.py: b**(-n) is printed as SBM_RCP(b)**n)
                v = sympy.Pow(args[0], -1)
            elif isinstance(node, sympy.core.function.AppliedUndef):
                raise _NotZero(node)
            else:
                v = node.func(*args)
        if v.free_symbols or v.is_finite is not True:
            raise _NotZero(node)
        seen[node] = v
        return v
    return value(f)


def f_zero_off_row(classes, share_products=False):
    """Whether EVERY class body gives f == 0 exactly, with no 0/0 and no reciprocal of 0 on the way, when all its
    parameter and state operands are 0 (``RL_F_ZERO_OFF_ROW`` of the model header).  The row-group kernels then give the
    lanes that evaluate no row such operands instead of zeroing their f with a select after every evaluation.  Decided
    on the expressions ``class_dispatch`` prints (the classes' CSE forms; a shared operation of the hoist is an operation
    of each class it serves, on that class's operands)."""
    for ci, c in enumerate(classes):
        repl, red = _class_cse(ci, c['canon'], share_products)
        try:
            if _f_at_zero_operands(repl, red[0]) != 0:
                return False
        except _NotZero:
            return False
    return True


def _dispatch_body(classes, n_slots, make_printer, hoist=True, share_products=False, memo=None):
    """The statements of ``class_dispatch``.  ``share_products``: a product that is a whole output of a class and also a
    group of factors of another of its outputs becomes a temporary of the class (``_share_products``)."""
    smap = {'t': 't'}
    for s in range(n_slots['ys']):
        smap['YS_%d' % s] = 'ys[%d]' % s
    for s in range(n_slots['ps']):
        smap['PS_%d' % s] = 'ps[%d]' % s
    pr = make_printer(smap)
    # Branch-free: every class body is evaluated on every lane (a divergent if/else chain would
    # execute all bodies one after the other anyway) and the lane keeps the results of ITS class
    # through by-value selects.  No per-lane control flow is left in the kernel, which matters
    # because other lanes read these registers with v_readlane.  The LAST class is the default of
    # the select chain (n-1 selects per output instead of n): lanes without a row (cls = -1) end up
    # with its values, which the kernels discard (spare LDS slots) or zero (f).
    L = []
    last = len(classes) - 1
    for ci in range(last):
        L.append("    const bool is%d = (cls == %d);" % (ci, ci))
    is_last_at = len(L)   # (the last class is the default of the output chains; a shared operand may still select on it)
    def class_cse(ci, canon):
        key = (ci, canon, share_products)
        if memo is not None and key in memo:
            return memo[key]
        repl, red = _class_cse(ci, canon, share_products)
        if memo is not None:
            memo[key] = (repl, red)
        return repl, red
    per_class = [class_cse(ci, c['canon']) for ci, c in enumerate(classes)]
    shared, hoisted = _plan_hoist(per_class, pr) if hoist and len(classes) > 1 else ([{} for _ in classes], [])
    # statements by name: the classes' CSE temporaries in their own order, a shared operation right before its first
    # use -- with the temporaries of OTHER classes that feed it pulled ahead of it
    stmts = OrderedDict()
    for ci, (repl, _) in enumerate(per_class):
        pr.shared = shared[ci]
        for sym, e in repl:
            stmts[str(sym)] = "    const double %s = %s;" % (sym, pr.doprint(e))
    for h in hoisted:
        stmts[h['name']] = "    const double %s = %s;   // classes %s" % (
            h['name'], _sel_template(h), ", ".join(str(ci) for ci in h['classes']))
    emitted = set()

    def emit_stmt(name):
        if name in emitted:
            return
        emitted.add(name)
        for dep in _NAME.findall(stmts[name].split('=', 1)[1]):
            if dep in stmts:
                emit_stmt(dep)
        L.append(stmts[name])

    bodies = []
    for ci, c in enumerate(classes):
        L.append("    // class %d: rows %s" % (ci, ", ".join(str(r) for r in c['rows'])))
        pr.shared = shared[ci]
        for sym, _ in per_class[ci][0]:
            emit_stmt(str(sym))
        bodies.append([pr.doprint(e) for e in per_class[ci][1]])
    pr.shared = {}
    for h in hoisted:   # (those the outputs use directly)
        emit_stmt(h['name'])
    if any("(is%d," % last in ln for ln in L[is_last_at:]):
        L.insert(is_last_at, "    const bool is%d = (cls == %d);" % (last, last))

    def chain(kind, k):
        """value of output (kind, k): the last class's expression (or 0), overridden class by class; a text all classes
        agree on is the value as it stands"""
        def of(ci):
            c = classes[ci]
            if kind == 'f':
                return bodies[ci][0]
            if kind == 'jy':
                return bodies[ci][1 + c['jy_slot'].index(k)] if k in c['jy_slot'] else "0.0"
            return bodies[ci][1 + c['n_jy'] + c['jp_slot'].index(k)] if k in c['jp_slot'] else "0.0"
        expr = of(last)
        if all(of(ci) == expr for ci in range(last)):
            return expr
        for ci in range(last - 1, -1, -1):
            expr = "SBM_SEL(is%d, %s, %s)" % (ci, of(ci), expr)
        return expr

    L.append("    f = %s;" % chain('f', 0))
    for k in range(n_slots['jy']):
        L.append("    jy[%d] = %s;" % (k, chain('jy', k)))
    for k in range(n_slots['jp']):
        L.append("    jp[%d] = %s;" % (k, chain('jp', k)))
    return L


def emit_rowlane_members(spec, d, meta, make_printer, hoist=True):
    """Member functions of ``struct SbmModel`` for the row-lane kernel.  ``hoist=False``: every class body in full
    (the reference form the shared one is checked against, tests/test_class_hoist.py)."""
    n = spec.n_vars
    classes = meta['classes']
    L = ["  // ---- row-lane form (sbm_sens_rowlane_kernel) ----",
         "  static constexpr int RL_NCLASS = %d;" % len(classes),
         "  static constexpr int RL_MAXYS = %d, RL_MAXPS = %d, RL_MAXJY = %d, RL_MAXJP = %d;"
         % (meta['max_ys'], meta['max_ps'], meta['max_jy'], meta['max_jp']),
         "  static constexpr int RL_LARGEST_CLASS = %d;  // rows evaluated side by side" %
         max(len(c['rows']) for c in classes),
         "  // every class body gives f == 0 exactly on all-zero operands (no select for lanes without a row)",
         "  static constexpr bool RL_F_ZERO_OFF_ROW = %s;" %
         ('true' if f_zero_off_row(classes, meta.get('share_products', False)) else 'false'),
         "  // table accessors (the tables are namespace-scope __constant__ arrays above)",
         "  __device__ __forceinline__ static int rl_class(int row) { return SBM_RL_CLASS[row]; }",
         "  __device__ __forceinline__ static int rl_ys(int slot, int row) { return SBM_RL_YS[slot * NV + row]; }",
         "  __device__ __forceinline__ static int rl_ps(int slot, int row) { return SBM_RL_PS[slot * NV + row]; }",
         "  __device__ __forceinline__ static int rl_jyout(int slot, int row) { return SBM_RL_JYOUT[slot * NV + row]; }",
         "  __device__ __forceinline__ static int rl_apos(int slot, int row) { return SBM_RL_APOS[slot * NV + row]; }",
         "  __device__ __forceinline__ static int rl_jpcol(int slot, int row) { return SBM_RL_JPCOL[slot * NV + row]; }",
         "  __device__ __forceinline__ static int rl_jycol(int slot, int row) { return SBM_RL_JYCOL[slot * NV + row]; }",
         "  // one class body per distinct kinetic form; lane = row, operands per lane",
         "  __device__ __forceinline__ static void class_dispatch(int cls, double t, const double (&ys)[RL_MAXYS],",
         "                                                        const double (&ps)[RL_MAXPS], double& f,",
         "                                                        double (&jy)[RL_MAXJY], double (&jp)[RL_MAXJP]) {",
         "    (void)t; (void)ys; (void)ps;"]
    L += _dispatch_body(classes, dict(ys=meta['max_ys'], ps=meta['max_ps'], jy=meta['max_jy'], jp=meta['max_jp']),
                        make_printer, hoist=hoist, share_products=meta.get('share_products', False))
    # which (row lane, slot) holds J_y non-zero e; entries that depend on parameters only are
    # STATIC: the same for every stage of every step, broadcast once per kernel (rl_static)
    where = {}
    for i in range(n):
        for k, (e_idx, c) in enumerate(d.jy_rows[i]):
            where[e_idx] = (i, k)
    var_names = set(spec.variables)
    static_idx = {}
    for e_idx in sorted(where):
        syms = {str(x) for x in d.jy_c[e_idx].free_symbols}
        if not (syms & var_names) and 't' not in syms:
            static_idx[e_idx] = len(static_idx)
    nst = max(len(static_idx), 1)
    L += ["  }", "",
          "  static constexpr int RL_NSTATIC = %d;   // J_y entries that depend on parameters only" % len(static_idx),
          "  // run once per kernel, after one class_dispatch: broadcast the static entries",
          "  __device__ __forceinline__ static void rl_static(const double (&jy)[RL_MAXJY], double (&sj)[%d]) {" % nst,
          "    (void)jy;"]
    if not static_idx:
        L.append("    sj[0] = 0.0;")
    for e_idx, si in static_idx.items():
        r, k = where[e_idx]
        L.append("    sj[%d] = SBM_LANE_BCAST(jy[%d], %d);" % (si, k, r))
    L += ["  }", "",
          "  // dz = J_y z + acol, one sensitivity column per lane.  A state-dependent J_y[i,m] sits in",
          "  // register jy[slot] of row lane i: SBM_LANE_BCAST (v_readlane, literal lane) turns it into a",
          "  // scalar operand; static entries come from sj; acol[i] = A[i][lane] was fetched from LDS.",
          "  template <int NZ>",
          "  __device__ __forceinline__ static void apply_rowlane(const double (&jy)[RL_MAXJY], const double (&sj)[%d]," % nst,
          "                                                       const double (&acol)[NV], const double (&z)[NZ],",
          "                                                       double (&dz)[NZ]) {",
          "    (void)jy; (void)sj;"]
    for i in range(n):
        expr = "acol[%d]" % i
        for e_idx, c in d.jy_base[i]:        # (summed in the order of the rows before alignment)
            if e_idx in static_idx:
                expr = "fma(sj[%d], z[%d], %s)" % (static_idx[e_idx], c, expr)
            else:
                r, k = where[e_idx]
                expr = "fma(SBM_LANE_BCAST(jy[%d], %d), z[%d], %s)" % (k, r, c, expr)
        L.append("    dz[%d] = %s;" % (i, expr))
    L += ["  }", "",
          "  // the same product with the J_y entries read from a table jyl[row * RL_MAXJY + slot] (LDS): the form of the",
          "  // packed kernel, where several trajectories share a wavefront and a lane cannot name its row lane literally",
          "  template <int NZ>",
          "  __device__ __forceinline__ static void apply_lds(const double* jyl, const double (&acol)[NV],",
          "                                                   const double (&z)[NZ], double (&dz)[NZ]) {",
          "    (void)jyl;"]
    for i in range(n):
        expr = "acol[%d]" % i
        for e_idx, c in d.jy_base[i]:
            expr = "fma(jyl[%d], z[%d], %s)" % (i * meta['max_jy'] + where[e_idx][1], c, expr)
        L.append("    dz[%d] = %s;" % (i, expr))
    L += ["  }"]
    return L
