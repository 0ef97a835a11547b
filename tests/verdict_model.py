"""The contract of the verifiers' verdict calls (include/hbmpc_hip.h: hbmpc_dev_check_degree, _check_top_coeff[_columns],
_check_double_share, _check_double_share_sel, _check_double_share_c0[_columns]) in plain Python.

Field elements are Python ints (any non-negative integer: the calls only ask "zero?" and "equal?", never reduce), status
bytes are ints.  Every check takes the arrays plus the incoming bad = [count, first] and returns the outgoing pair:

  count += number of failing entries
  first  = min(first, lowest failing entry)                 columns == 0
  first  = min(first, lowest failing entry mod columns)     columns > 0: several verifiers' results over the same columns,
                                                            one verifier after the other -- the lowest failing COLUMN

The caller starts from bad = [0, 0xffffffff]."""
FRESH = (0, 0xFFFFFFFF)


def degree(coeffs):
    """DensePolynomial::degree() of an untrimmed coefficient list: index of the highest non-zero coefficient, 0 for the zero polynomial"""
    for k in range(len(coeffs) - 1, 0, -1):
        if coeffs[k] != 0:
            return k
    return 0


def status_fails(st):
    """a chunk's status byte: 0 (clean) and 1 (repaired by the fallback) are successes, everything else a failed reconstruction"""
    return st > 1


def accumulate(failing, bad=FRESH, columns=0):
    """the count rule and the first rule over a list of booleans, one per entry"""
    idx = [g for g, f in enumerate(failing) if f]
    if columns:
        assert len(failing) % columns == 0
        idx = [g % columns for g in idx]
    return [bad[0] + len(idx), min([bad[1]] + idx)]


def check_degree(coeffs, status, want, bad=FRESH):
    """coeffs[G][m]; status[G] or None"""
    return accumulate([(status is not None and status_fails(status[g])) or degree(c) != want for g, c in enumerate(coeffs)], bad)


def check_top_coeff(top, status, want, bad=FRESH, columns=0):
    """top[G] = coefficient `want` of polynomials of at most want + 1 coefficients; want = 0 leaves the status test"""
    return accumulate([(status is not None and status_fails(status[g])) or (want > 0 and x == 0) for g, x in enumerate(top)], bad, columns)


def check_double_share(ct, c2t, t, bad=FRESH):
    """ct[G][m], c2t[G][m]: degree t, degree 2t, equal constant terms"""
    return accumulate([degree(a) != t or degree(b) != 2 * t or a[0] != b[0] for a, b in zip(ct, c2t)], bad)


def check_double_share_sel(sel_t, st_t, sel_2t, st_2t, t, bad=FRESH, columns=0):
    """sel_*[G] = (constant term, top coefficient) of hbmpc_dev_interpolate_degree_check_strided, st_*[G] its status"""
    return accumulate([status_fails(sa) or status_fails(sb) or (t > 0 and (a[1] == 0 or b[1] == 0)) or a[0] != b[0]
                       for a, sa, b, sb in zip(sel_t, st_t, sel_2t, st_2t)], bad, columns)


def check_double_share_c0(c0_t, deg_t, c0_2t, deg_2t, t, bad=FRESH, columns=0):
    """c0_*[G], deg_*[G] of hbmpc_dev_batch_interpolate_c0; columns = 0 is hbmpc_dev_check_double_share_c0"""
    return accumulate([da != t or db != 2 * t or a != b for a, da, b, db in zip(c0_t, deg_t, c0_2t, deg_2t)], bad, columns)
