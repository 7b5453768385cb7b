"""L-BFGS with a More-Thuente line search: the algorithm sklearn's ``LogisticRegression(solver="lbfgs")`` reaches through L-BFGS-B when no
variable is bounded, written from the published descriptions (Liu & Nocedal 1989, the two-loop recursion; Byrd, Lu, Nocedal & Zhu 1995, the
stopping rules and the restart after a failed search; More & Thuente 1994, the line search and its safeguarded step).

Vectors (iterate, gradient, history) are float64 tensors on the evaluator's device; every decision is taken in double on the host.  An
evaluator is any object with ``value_and_grad(x64) -> (f, g64)``, f a Python float or a 0-dim float64 tensor.  One evaluation costs ONE host
synchronisation: f, max|g| and every dot product the line search, the pair test and the two-loop recursion need come to the host in one
transfer.  The recursion itself runs on the host over the Gram matrix of the kept pairs; a new direction is one small upload and one product.

``TorchLogistic`` is the float64 evaluator of the linear probe's objective (mudpt_amd/lpclip.py) on any device; the HIP evaluator lives next to
the kernels' binding in lpclip.py.
"""
from __future__ import annotations

import numpy as np
import torch

EPS64 = float(np.finfo(np.float64).eps)
FTOL, GTOL, XTOL = 1e-3, 0.9, 0.1  # sufficient decrease, curvature, relative width of the bracket
STPMAX = 1e10
MAX_TRIALS = 50       # evaluations per line search
MAX_EVALS = 15000
MEMORY = 10
FACTR = 64.0          # f_k - f_{k+1} <= FACTR * eps64 * max(|f_k|, |f_{k+1}|, 1)

CONVERGED_GRADIENT, CONVERGED_DECREASE, STOPPED_ITERATIONS, STOPPED_EVALUATIONS, FAILED_LINE_SEARCH = range(5)
STATUS = ("max|g| <= tol", "relative decrease of f below 64 eps", "max_iter reached", "evaluation limit reached", "line search failed twice")


def _safeguarded_step(stx, fx, dx, sty, fy, dy, stp, fp, dp, brackt, stpmin, stpmax):
    """More & Thuente 1994, section 4: the trial step from the best step so far (stx), the other endpoint (sty) and the current trial (stp),
    by the minimisers of the cubic through (fx, dx, fp, dp) and of the two quadratics.  Returns the new (stx, fx, dx, sty, fy, dy, stp, brackt)."""
    sgnd = dp * (dx / abs(dx))
    if fp > fx:  # case 1: a higher value: the minimum is bracketed
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        s = max(abs(theta), abs(dx), abs(dp))
        gamma = s * np.sqrt((theta / s) ** 2 - (dx / s) * (dp / s))
        if stp < stx:
            gamma = -gamma
        p, q = (gamma - dx) + theta, ((gamma - dx) + gamma) + dp
        r = p / q
        stpc = stx + r * (stp - stx)
        stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / 2.0) * (stp - stx)
        stpf = stpc if abs(stpc - stx) < abs(stpq - stx) else stpc + (stpq - stpc) / 2.0
        brackt = True
    elif sgnd < 0.0:  # case 2: a lower value and derivatives of opposite sign: bracketed
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        s = max(abs(theta), abs(dx), abs(dp))
        gamma = s * np.sqrt((theta / s) ** 2 - (dx / s) * (dp / s))
        if stp > stx:
            gamma = -gamma
        p, q = (gamma - dp) + theta, ((gamma - dp) + gamma) + dx
        r = p / q
        stpc = stp + r * (stx - stp)
        stpq = stp + (dp / (dp - dx)) * (stx - stp)
        stpf = stpc if abs(stpc - stp) > abs(stpq - stp) else stpq
        brackt = True
    elif abs(dp) < abs(dx):  # case 3: a lower value, same sign, the derivative shrinks
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        s = max(abs(theta), abs(dx), abs(dp))
        gamma = s * np.sqrt(max(0.0, (theta / s) ** 2 - (dx / s) * (dp / s)))
        if stp > stx:
            gamma = -gamma
        p, q = (gamma - dp) + theta, (gamma + (dx - dp)) + gamma
        r = p / q
        if r < 0.0 and gamma != 0.0:
            stpc = stp + r * (stx - stp)
        elif stp > stx:
            stpc = stpmax
        else:
            stpc = stpmin
        stpq = stp + (dp / (dp - dx)) * (stx - stp)
        if brackt:
            stpf = stpc if abs(stpc - stp) < abs(stpq - stp) else stpq
            stpf = min(stp + 0.66 * (sty - stp), stpf) if stp > stx else max(stp + 0.66 * (sty - stp), stpf)
        else:
            stpf = stpc if abs(stpc - stp) > abs(stpq - stp) else stpq
            stpf = max(stpmin, min(stpmax, stpf))
    else:  # case 4: a lower value, same sign, the derivative does not shrink
        if brackt:
            theta = 3.0 * (fp - fy) / (sty - stp) + dy + dp
            s = max(abs(theta), abs(dy), abs(dp))
            gamma = s * np.sqrt((theta / s) ** 2 - (dy / s) * (dp / s))
            if stp > sty:
                gamma = -gamma
            p, q = (gamma - dp) + theta, ((gamma - dp) + gamma) + dy
            r = p / q
            stpf = stp + r * (sty - stp)
        elif stp > stx:
            stpf = stpmax
        else:
            stpf = stpmin
    if fp > fx:
        sty, fy, dy = stp, fp, dp
    else:
        if sgnd < 0.0:
            sty, fy, dy = stx, fx, dx
        stx, fx, dx = stp, fp, dp
    return stx, fx, dx, sty, fy, dy, stpf, brackt


class LineSearch:
    """More & Thuente's search for a step with f(stp) <= f(0) + ftol stp f'(0) and |f'(stp)| <= gtol |f'(0)|, as a state machine: ``start``
    takes f(0), f'(0) < 0 and the first trial; ``advance(f, g)`` takes the values at ``self.stp`` and returns None (evaluate the new
    ``self.stp``), "converged" or a warning -- the bracket narrower than xtol, rounding, a bound reached.  A warning ends the search AT the
    step just evaluated, as L-BFGS-B does."""

    def __init__(self, ftol=FTOL, gtol=GTOL, xtol=XTOL, stpmin=0.0, stpmax=STPMAX):
        self.ftol, self.gtol, self.xtol, self.stpmin, self.stpmax = ftol, gtol, xtol, stpmin, stpmax

    def start(self, f0, g0, stp):
        assert g0 < 0.0 and self.stpmin <= stp <= self.stpmax
        self.brackt, self.stage = False, 1
        self.finit, self.ginit, self.gtest = f0, g0, self.ftol * g0
        self.width = self.stpmax - self.stpmin
        self.width1 = 2.0 * self.width
        self.stx, self.fx, self.gx = 0.0, f0, g0
        self.sty, self.fy, self.gy = 0.0, f0, g0
        self.stmin, self.stmax = 0.0, stp + 4.0 * stp
        self.stp = stp

    def advance(self, f, g):
        stp = self.stp
        ftest = self.finit + stp * self.gtest
        if self.stage == 1 and f <= ftest and g >= 0.0:
            self.stage = 2
        verdict = None
        if self.brackt and (stp <= self.stmin or stp >= self.stmax):
            verdict = "rounding errors prevent progress"
        if self.brackt and self.stmax - self.stmin <= self.xtol * self.stmax:
            verdict = "bracket narrower than xtol"
        if stp == self.stpmax and f <= ftest and g <= self.gtest:
            verdict = "step at its upper bound"
        if stp == self.stpmin and (f > ftest or g >= self.gtest):
            verdict = "step at its lower bound"
        if f <= ftest and abs(g) <= self.gtol * (-self.ginit):
            verdict = "converged"
        if verdict is not None:
            return verdict
        if self.stage == 1 and f <= self.fx and f > ftest:  # the modified function of the first stage
            gt = self.gtest
            out = _safeguarded_step(self.stx, self.fx - self.stx * gt, self.gx - gt, self.sty, self.fy - self.sty * gt, self.gy - gt,
                                    stp, f - stp * gt, g - gt, self.brackt, self.stmin, self.stmax)
            self.stx, fxm, gxm, self.sty, fym, gym, stp, self.brackt = out
            self.fx, self.fy, self.gx, self.gy = fxm + self.stx * gt, fym + self.sty * gt, gxm + gt, gym + gt
        else:
            out = _safeguarded_step(self.stx, self.fx, self.gx, self.sty, self.fy, self.gy, stp, f, g, self.brackt, self.stmin, self.stmax)
            self.stx, self.fx, self.gx, self.sty, self.fy, self.gy, stp, self.brackt = out
        if self.brackt:
            if abs(self.sty - self.stx) >= 0.66 * self.width1:
                stp = self.stx + 0.5 * (self.sty - self.stx)
            self.width1, self.width = self.width, abs(self.sty - self.stx)
            self.stmin, self.stmax = min(self.stx, self.sty), max(self.stx, self.sty)
        else:
            self.stmin, self.stmax = stp + 1.1 * (stp - self.stx), stp + 4.0 * (stp - self.stx)
        stp = min(max(stp, self.stpmin), self.stpmax)
        if self.brackt and (stp <= self.stmin or stp >= self.stmax or self.stmax - self.stmin <= self.xtol * self.stmax):
            stp = self.stx
        self.stp = stp
        return None


class Result:
    def __init__(self, x, f, n_iter, n_eval, status, max_grad, searches):
        self.x, self.f, self.n_iter, self.n_eval, self.status, self.max_grad, self.searches = x, f, n_iter, n_eval, status, max_grad, searches
        self.message = STATUS[status]
        self.converged = status in (CONVERGED_GRADIENT, CONVERGED_DECREASE)


class _Memory:
    """The kept pairs as rows of ONE device matrix (s_i in row slot, y_i in row memory + slot) and, on the host, the Gram matrix of those
    rows and the current gradient (index 2 memory).  The two-loop recursion then runs on the host over coefficient vectors (Chen et al. 2014,
    "vector-free" L-BFGS: every dot product s_i.q or y_i.q of the recursion is a combination of Gram entries), and the direction is one
    product coefficients @ rows on the device."""

    def __init__(self, memory, n, device):
        self.m = memory
        # rows 2m .. 2m + 3: the vectors of the evaluation under way (g, y = g - g_prev, d, g_prev), so that every product the host needs is
        # rows @ one of them -- three matrix-vector products (a [20, n] x [n, 3] product is a GEMM with one output tile and a reduction of
        # n = 513 000: measured 82 ms on the MI355X against 0.07 ms for the three products)
        self.rows = torch.zeros(2 * memory + 4, n, dtype=torch.float64, device=device)
        self.gram = np.zeros((2 * memory + 1, 2 * memory + 1))
        self.slots = []  # row slots of the kept pairs, oldest first
        self.gamma = 1.0

    def clear(self):
        self.slots, self.gamma = [], 1.0
        self.rows[:2 * self.m].zero_()  # a dropped row still enters rows @ v and the Gram sums with coefficient 0: it must stay finite
        self.gram[:] = 0.0

    def coefficients(self):
        """delta with -H g = delta[:2m] @ rows + delta[2m] g"""
        m, G = self.m, self.gram
        delta = np.zeros(2 * m + 1)
        delta[2 * m] = -1.0
        alpha = {}
        for i in reversed(self.slots):
            alpha[i] = float(delta @ G[:, i]) / G[i, m + i]
            delta[m + i] -= alpha[i]
        delta *= self.gamma
        for i in self.slots:
            beta = float(delta @ G[:, m + i]) / G[i, m + i]
            delta[i] += alpha[i] - beta
        return delta

    def new_gradient(self, g_rows, gg):
        """the Gram row of the gradient after a step: g_rows = rows @ g, gg = g.g"""
        k = 2 * self.m
        self.gram[k, :k] = self.gram[:k, k] = g_rows
        self.gram[k, k] = gg

    def push(self, d, stp, y, d_rows, y_rows, dd, dy, yy, gd, gy):
        """keep the pair s = stp d, y; *_rows = rows @ that vector BEFORE the pair is stored, gd / gy = (new gradient) . d / y"""
        m = self.m
        slot = self.slots.pop(0) if len(self.slots) == m else next(i for i in range(m) if i not in self.slots)
        torch.mul(d, stp, out=self.rows[slot])
        self.rows[m + slot].copy_(y)  # y: row 2m + 1, still the accepted trial's
        G = self.gram
        for r, vec_rows in ((slot, stp * np.asarray(d_rows)), (m + slot, np.asarray(y_rows))):
            G[r, :2 * m] = G[:2 * m, r] = vec_rows
        G[slot, slot], G[m + slot, m + slot] = stp * stp * dd, yy
        G[slot, m + slot] = G[m + slot, slot] = stp * dy
        G[2 * m, slot] = G[slot, 2 * m] = stp * gd
        G[2 * m, m + slot] = G[m + slot, 2 * m] = gy
        self.slots.append(slot)
        self.gamma = stp * dy / yy


def minimize(evaluator, x0, tol=1e-4, max_iter=1000, memory=MEMORY, max_trials=MAX_TRIALS, max_evals=MAX_EVALS, record=False):
    """Minimise from x0 (float64).  Stops when max|g| <= tol (tested at x0 too), when f_k - f_{k+1} <= 64 eps max(|f_k|, |f_{k+1}|, 1), after
    max_iter iterations or max_evals evaluations.  A line search that fails (no descent direction, or max_trials evaluations without an
    accepted step) drops the memory and restarts from steepest descent at the last iterate; failing there too ends the run with
    FAILED_LINE_SEARCH.  record: keep (f0, g0.d, stp, f, g.d, verdict, trials) of every accepted step in Result.searches."""
    x = x0.detach().clone().to(torch.float64)
    mem = _Memory(memory, x.numel(), x.device)
    m2 = 2 * memory

    def evaluate(xt, d, g_prev):
        """f and g at xt and, in ONE transfer (the one host synchronisation of an evaluation): f, max|g|, and the products of the kept
        rows and of (g, y = g - g_prev, d, g_prev) with (g, y, d) -- every scalar the line search, the pair test and the Gram matrix need"""
        f, g = evaluator.value_and_grad(xt)
        f = f.to(torch.float64) if torch.is_tensor(f) else torch.tensor(float(f), dtype=torch.float64, device=xt.device)
        if d is None:
            return g, torch.stack([f.reshape(()), g.abs().max(), torch.dot(g, g)]).tolist(), None, None
        W = mem.rows  # rows m2 + 2 (d) and m2 + 3 (g_prev) were set when the direction was made
        W[m2].copy_(g)
        torch.sub(g, g_prev, out=W[m2 + 1])
        prod = torch.stack([torch.mv(W, W[m2]), torch.mv(W, W[m2 + 1]), torch.mv(W, W[m2 + 2])], dim=1)  # [2m + 4, 3]
        flat = torch.cat([f.reshape(1), g.abs().max().reshape(1), prod.reshape(-1)]).tolist()
        prod = np.array(flat[2:]).reshape(m2 + 4, 3)
        return g, flat[:2], prod[:m2], (prod[m2:], W[m2 + 1])

    g, (f, gmax, gg), _, _ = evaluate(x, None, None)
    n_eval, n_iter, searches = 1, 0, []
    if gmax <= tol:
        return Result(x, f, 0, n_eval, CONVERGED_GRADIENT, gmax, searches)
    mem.new_gradient(np.zeros(m2), gg)
    first = True
    while True:
        if mem.slots:
            delta = mem.coefficients()
            d = torch.mv(mem.rows[:m2].t(), torch.as_tensor(delta[:m2], device=x.device))
            d.add_(g, alpha=float(delta[m2]))
        else:
            d = g.neg()
        mem.rows[m2 + 2].copy_(d)
        mem.rows[m2 + 3].copy_(g)
        # the first trial: 1 / |d| on the very first search (d = -g there), 1 afterwards.  The slope g.d comes back with the first trial's
        # scalars, so a direction that is no descent direction costs one wasted evaluation
        ls = LineSearch()
        stp = min(1.0 / np.sqrt(gg), STPMAX) if first else 1.0
        trials, failed, verdict = 0, False, None
        while verdict is None:
            if trials >= max_trials:
                failed = True
                break
            xt = torch.add(x, d, alpha=stp)
            gt, (ft, gmax_t), rows_dot, (vv, y) = evaluate(xt, d, g)
            trials += 1
            n_eval += 1
            gdt, gd0 = vv[0, 2], vv[3, 2]
            if trials == 1:
                if gd0 >= 0.0:
                    failed = True
                    break
                ls.start(f, gd0, stp)
            verdict = ls.advance(ft, gdt)
            stp = ls.stp
        if failed:
            if not mem.slots:
                return Result(x, f, n_iter, n_eval, FAILED_LINE_SEARCH, gmax, searches)
            mem.clear()  # drop the memory, go on from x along -g with a unit first step
            continue
        first = False
        if record:
            searches.append((f, gd0, stp, ft, gdt, verdict, trials))
        f_old = f
        x, f, g, gmax, gg = xt, ft, gt, gmax_t, vv[0, 0]
        n_iter += 1
        if n_iter >= max_iter:
            return Result(x, f, n_iter, n_eval, STOPPED_ITERATIONS, gmax, searches)
        if n_eval > max_evals:
            return Result(x, f, n_iter, n_eval, STOPPED_EVALUATIONS, gmax, searches)
        if gmax <= tol:
            return Result(x, f, n_iter, n_eval, CONVERGED_GRADIENT, gmax, searches)
        if f_old - f <= FACTR * EPS64 * max(abs(f_old), abs(f), 1.0):
            return Result(x, f, n_iter, n_eval, CONVERGED_DECREASE, gmax, searches)
        dy, yy = vv[1, 2], vv[1, 1]
        mem.new_gradient(rows_dot[:, 0], gg)
        if stp * dy > EPS64 * yy:  # s.y > eps y.y, s = stp d
            mem.push(d, stp, y, rows_dot[:, 2], rows_dot[:, 1], vv[2, 2], dy, yy, vv[0, 2], vv[0, 1])


class TorchLogistic:
    """The probe's objective in float64 torch on any device (the reference is a float64 computation: sklearn converts fp32 features for this
    solver).  x = [W.ravel(), b];  F = (1/N) sum_i [logsumexp(z_i) - z_i[y_i]] + |W|^2 / (2 C N), z = X W^T + b; C is rounded to fp32 first, as
    it is wherever it travels to a kernel."""

    def __init__(self, X, y, n_cls, C):
        self.X = X.to(torch.float64)
        self.y = y.to(torch.int64)
        self.N, self.K = self.X.shape
        self.n_cls = n_cls
        self.reg = 1.0 / (float(np.float32(C)) * self.N)
        self.rows = torch.arange(self.N, device=self.X.device)

    def numel(self):
        return self.n_cls * (self.K + 1)

    def value_and_grad(self, x):
        nW = self.n_cls * self.K
        W, b = x[:nW].view(self.n_cls, self.K), x[nW:]
        Z = torch.addmm(b, self.X, W.t())
        lse = torch.logsumexp(Z, dim=1)
        f = (lse - Z[self.rows, self.y]).sum() / self.N + 0.5 * self.reg * (W * W).sum()
        P = torch.exp(Z - lse[:, None])
        P[self.rows, self.y] -= 1.0
        P /= self.N
        return f, torch.cat([(P.t() @ self.X + self.reg * W).reshape(-1), P.sum(0)])
