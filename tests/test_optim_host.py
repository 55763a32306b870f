"""The optimizer entry points of include/cdml.h (csrc/optim.hip), host side: every argument check answers with its own
return code before anything is launched, so none of this needs a GPU.  The pointers are fake and never dereferenced; the
segment arrays are host arrays, which the library does read."""
import ctypes as C

BADARG, ALIGN, UNSUPPORTED = -1, -3, -4
P, ODD = 4096, 4100                                      # a 16-B aligned address and one that is not
K, N = 128, 64


def _segs(pairs):
    n = len(pairs)
    return (C.c_int64 * n)(*[o for o, _ in pairs]), (C.c_int64 * n)(*[s for _, s in pairs])


def _entry(lib, name, fields, **defaults):
    """case(**changes) -> (name, changes, return code) of the entry called with its valid defaults and those changes."""
    fields = fields.split()
    assert len(fields) == len(getattr(lib, name).argtypes) and set(defaults) <= set(fields), name

    def case(**kw):
        assert set(kw) <= set(fields), (name, kw)
        a = dict(dict.fromkeys(fields, None), **defaults)
        a.update(kw)
        return name, kw, getattr(lib, name)(*[a[f] for f in fields])
    return case


def test_argument_errors_need_no_gpu():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    lib = _lib.load_library()
    assert lib.cdml_version() == 3000 and isinstance(lib.cdml_last_error(), bytes)
    assert lib.cdml_lars_scratch_floats() == 2 + 2 * 1024 and lib.cdml_lars_multi_scratch_floats() == 2 * 1024
    p, odd = C.c_void_p(P), C.c_void_p(ODD)
    got = []

    def expect(code, *cases):
        got.extend((name, kw, rc, code) for name, kw, rc in cases)

    # ---- the flat kernels ----
    adam = _entry(lib, "cdml_adam_step", "w g m v n lr lr_dev b1 b2 eps t t_dev adv tickets stream",
                  w=p, g=p, m=p, v=p, n=1000, lr=0.01, b1=0.9, b2=0.999, eps=1e-8, t=1, adv=0)
    expect(BADARG, adam(w=None), adam(g=None), adam(m=None), adam(v=None), adam(n=0), adam(n=-4),
           adam(adv=1), adam(adv=1, t_dev=p), adam(adv=1, tickets=p), adam(t=0), adam(t=-1, t_dev=p),
           adam(t=0, w=odd))                             # (the step check fires before the alignment check)
    expect(ALIGN, adam(w=odd), adam(g=odd), adam(m=odd), adam(v=odd))
    lars = _entry(lib, "cdml_lars_step", "w g acc n lr lr_dev momentum wd eeta eps scratch stream",
                  w=p, g=p, acc=p, n=1000, lr=0.01, momentum=0.9, wd=1e-4, eeta=1e-3, eps=0.0, scratch=p)
    expect(BADARG, lars(w=None), lars(g=None), lars(acc=None), lars(scratch=None), lars(n=0))
    prep = _entry(lib, "cdml_grad_prepare", "g w n l2 clip scratch norms stream", g=p, w=p, n=1000, l2=0.0, clip=1.0, scratch=p)
    expect(BADARG, prep(g=None), prep(w=None), prep(scratch=None), prep(n=0))
    mom = _entry(lib, "cdml_momentum_step", "w g acc n lr lr_dev momentum nesterov stream",
                 w=p, g=p, acc=p, n=1000, lr=0.01, momentum=0.9, nesterov=1)
    expect(BADARG, mom(w=None), mom(g=None), mom(acc=None), mom(n=0))

    # ---- the segment layout: cdml_lars_multi, cdml_lars_multi_norms, cdml_lars_matrix(_h2) ----
    offs, sizes = _segs([(0, K * N), (K * N, N), (K * N + N, 4 * N)])
    nine = _segs([(4 * k, 4) for k in range(9)])
    gap = _segs([(0, K * N), (K * N + 4, N)])
    ragged = _segs([(0, K * N), (K * N, N + 2)])
    empty = _segs([(0, K * N), (K * N, 0)])

    def layout_cases(fn):
        expect(UNSUPPORTED, fn(n_seg=0), fn(offs=nine[0], sizes=nine[1], n_seg=9))
        expect(BADARG, fn(offs=gap[0], sizes=gap[1], n_seg=2), fn(offs=ragged[0], sizes=ragged[1], n_seg=2),
               fn(offs=empty[0], sizes=empty[1], n_seg=2), fn(offs=None), fn(sizes=None))

    multi = _entry(lib, "cdml_lars_multi", "w g acc offs sizes n_seg lr lr_dev momentum wd eeta eps scratch norms step tickets stream",
                   w=p, g=p, acc=p, offs=offs, sizes=sizes, n_seg=3, lr=0.01, momentum=0.9, wd=1e-4, eeta=1e-3, eps=0.0, scratch=p)
    expect(BADARG, multi(w=None), multi(g=None), multi(acc=None), multi(scratch=None), multi(step=p))
    expect(ALIGN, multi(w=odd), multi(g=odd), multi(acc=odd))
    layout_cases(multi)
    norms = _entry(lib, "cdml_lars_multi_norms", "w g offs sizes n_seg scratch stream", w=p, g=p, offs=offs, sizes=sizes, n_seg=3, scratch=p)
    expect(BADARG, norms(w=None), norms(g=None), norms(scratch=None))
    expect(ALIGN, norms(w=odd), norms(g=odd))
    layout_cases(norms)

    # ---- the operand copies, the same for every matrix rule: wt = W^T [N][ldt], wc = W [K][ldc], 1 / 2 / 3 planes ----
    def copies_cases(fn, planes, shape=True):
        """``fn`` has valid defaults for ``planes`` planes with plane strides K and N (shape: K and N are free arguments)."""
        if shape:
            expect(UNSUPPORTED, fn(K=96), fn(N=96))
        expect(ALIGN, fn(wt=odd), fn(wc=odd), fn(ldt=planes * K + 4), fn(ldc=planes * N + 2), fn(ldt=planes * K - 8), fn(ldc=planes * N - 4),
               fn(ldt=K - 8, wc=None), fn(ldc=N - 4, wt=None))
        if planes > 1:
            expect(ALIGN, fn(plane_t=K + 4, ldt=4 * K), fn(plane_c=N + 2, ldc=4 * N), fn(plane_t=K - 8), fn(plane_c=N - 4),
                   fn(plane_t=K + 8), fn(plane_c=N + 4), fn(plane_t=0), fn(plane_c=0))

    common = dict(w=p, g=p, m=p, v=p, K=K, N=N, lr=0.01, b1=0.9, b2=0.999, eps=1e-8, t=1, wt=p, wc=p, bn=0, adv=0)
    head = "w g m v K N lr lr_dev b1 b2 eps t t_dev "
    tail = " bw bg bm bv bn adv tickets stream"
    am1 = _entry(lib, "cdml_adam_matrix_bf16", head + "wt ldt wc ldc" + tail, ldt=K, ldc=N, **common)
    am3 = _entry(lib, "cdml_adam_matrix_planes", head + "wt ldt plane_t wc ldc plane_c" + tail,
                 ldt=3 * K, plane_t=K, ldc=3 * N, plane_c=N, **common)
    am2 = _entry(lib, "cdml_adam_matrix_h2", head + "wt ldt plane_t wc ldc plane_c scale" + tail,
                 ldt=2 * K, plane_t=K, ldc=2 * N, plane_c=N, scale=64.0, **common)
    for am, planes in ((am1, 1), (am2, 2), (am3, 3)):
        expect(BADARG, am(w=None), am(g=None), am(m=None), am(v=None), am(K=0), am(N=0), am(K=-64), am(K=0, N=96),
               am(bw=p), am(bw=p, bg=p, bm=p, bv=p), am(bw=p, bg=p, bm=p, bn=8), am(bw=p, bg=p, bv=p, bn=8), am(bw=p, bm=p, bv=p, bn=8),
               am(adv=1), am(adv=1, t_dev=p), am(adv=1, tickets=p), am(t=0), am(t=-1, t_dev=p),
               am(t=0, wt=odd), am(t=0, w=odd))          # (the step check fires before the alignment checks ...
        expect(UNSUPPORTED, am(t=0, K=96), am(K=96, wt=odd))   # ... and after the shape check)
        expect(ALIGN, am(w=odd), am(g=odd), am(m=odd), am(v=odd))
        copies_cases(am, planes)
    expect(ALIGN, am2(scale=0.0), am2(scale=-1.0))

    mm_common = dict(w=p, g=p, acc=p, K=K, N=N, lr=0.01, momentum=0.9, nesterov=1, wt=p, wc=p, bn=0)
    mm = _entry(lib, "cdml_momentum_matrix", "w g acc K N lr lr_dev momentum nesterov wt ldt plane_t wc ldc plane_c planes bw bg bacc bn "
                "step tickets stream", ldt=K, plane_t=0, ldc=N, plane_c=0, planes=1, **mm_common)
    mm3 = lambda **kw: mm(**dict(dict(ldt=3 * K, plane_t=K, ldc=3 * N, plane_c=N, planes=3), **kw))
    mm2 = _entry(lib, "cdml_momentum_matrix_h2", "w g acc K N lr lr_dev momentum nesterov wt ldt plane_t wc ldc plane_c scale bw bg bacc bn "
                 "step tickets stream", ldt=2 * K, plane_t=K, ldc=2 * N, plane_c=N, scale=64.0, **mm_common)
    expect(BADARG, mm(planes=0), mm(planes=2), mm(planes=4), mm(planes=2, ldt=2 * K, plane_t=K, ldc=2 * N, plane_c=N),
           mm2(scale=0.0), mm2(scale=-1.0))
    for fn, planes in ((mm, 1), (mm2, 2), (mm3, 3)):
        expect(BADARG, fn(w=None), fn(g=None), fn(acc=None), fn(bw=p), fn(bw=p, bg=p, bacc=p), fn(bw=p, bg=p, bn=8), fn(bw=p, bacc=p, bn=8),
               fn(step=p), fn(step=p, K=96))
        expect(UNSUPPORTED, fn(K=0), fn(N=0), fn(K=96, wt=odd))
        expect(ALIGN, fn(w=odd), fn(g=odd), fn(acc=odd), fn(w=odd, K=96))
        copies_cases(fn, planes)

    lm_common = dict(w=p, g=p, acc=p, offs=offs, sizes=sizes, n_seg=3, seg_m=0, seg_b=1, K=K, N=N, lr=0.01, momentum=0.9, wd=1e-4,
                     eeta=1e-3, eps=0.0, scratch=p, wt=p, wc=p)
    lm_head = "w g acc offs sizes n_seg seg_m seg_b K N lr lr_dev momentum wd eeta eps scratch norms wt ldt plane_t wc ldc plane_c "
    lm = _entry(lib, "cdml_lars_matrix", lm_head + "planes step tickets stream", ldt=K, plane_t=0, ldc=N, plane_c=0, planes=1, **lm_common)
    lm3 = lambda **kw: lm(**dict(dict(ldt=3 * K, plane_t=K, ldc=3 * N, plane_c=N, planes=3), **kw))
    lm2 = _entry(lib, "cdml_lars_matrix_h2", lm_head + "scale step tickets stream", ldt=2 * K, plane_t=K, ldc=2 * N, plane_c=N, scale=64.0,
                 **lm_common)
    expect(BADARG, lm(planes=0), lm(planes=2), lm(planes=4), lm(planes=2, ldt=2 * K, plane_t=K, ldc=2 * N, plane_c=N),
           lm2(scale=0.0), lm2(scale=-1.0))
    o96, s96 = _segs([(0, 96 * N), (96 * N, N)])
    k96, n96 = _segs([(0, K * 96), (K * 96, 96)])
    for fn, planes in ((lm, 1), (lm2, 2), (lm3, 3)):
        expect(BADARG, fn(w=None), fn(g=None), fn(acc=None), fn(scratch=None), fn(step=p),
               fn(seg_m=-1), fn(seg_m=3), fn(seg_b=3), fn(seg_b=0), fn(seg_m=1, seg_b=1),
               fn(seg_m=2), fn(K=64), fn(N=128), fn(K=96), fn(K=0))
        expect(ALIGN, fn(w=odd), fn(g=odd), fn(acc=odd), fn(w=odd, n_seg=0))
        layout_cases(fn)
        expect(UNSUPPORTED, fn(offs=o96, sizes=s96, n_seg=2, K=96), fn(offs=k96, sizes=n96, n_seg=2, N=96),
               fn(seg_m=1, seg_b=-1, K=1, N=N), fn(seg_m=1, seg_b=-1, K=N, N=1), fn(offs=o96, sizes=s96, n_seg=2, K=96, wt=odd))
        copies_cases(fn, planes, shape=False)             # (K x N is the segment's size: the cases above)
        copies_cases(lambda **kw: fn(**dict(dict(seg_b=-1), **kw)), planes, shape=False)

    names = {name for name, _, _, _ in got}
    assert len(names) == 13 and len(got) > 400
    wrong = [(name, kw, rc, code) for name, kw, rc, code in got if rc != code]
    assert not wrong, wrong
