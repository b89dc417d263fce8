"""What each launcher of sproxy_amd/csrc/md5_kernels.hip and md5_pages.hip must launch: the case
table of tests/test_launch_routes.py (no device: the real launchers over a
recording runtime) and tests/test_launch_routes_gpu.py (the same arguments on
the device, results against hashlib and zlib).

`cases(cus)` lists the cases for a device of `cus` compute units.  A case is
an entry of include/md5hip.h with its arguments, the return code and the
records the call must leave: which kernel, grid, block, dynamic LDS, stream
and kernel arguments, and for BALANCED its attribute call and memset before
the launch.  The expectation is restated here from md5hip.h's text and the
launchers' comments -- the route_* functions below -- and never comes from
calling the library.  Each case also names its kernel in words (`kernel=`),
and the table refuses to build when that and the route function disagree, so
a case cannot drift to another route unnoticed when a count scales with CUs.

The cases sit on both sides of every edge the launchers have: n = 0, each
-EINVAL, base and stride on and off the 16-B grid, the stride where 32-bit
offsets end (2^25), the group counts at CUs and CUs + 1, the two-block edge
of the fed pairs, every named variant, the CRC ladder's windows and their
sizes, 12, 16 and 128 chunks per CU, the grid caps, the one-pass kind's three
bounds, and the three paged entries' kinds, page sizes and group counts.  Test
infrastructure."""

EINVAL = -22
MAXGRID = 2**31 - 1                      # a launch's grid limit: a batch that needs more is -EINVAL
KMAX = 1 << 17                           # MD5HIP_HIST_KMAX
FEDSPLIT_MIN_LEN = 1024                  # MD5CRC32HIP_FEDSPLIT_MIN_LEN
FAR = 1 << 25                            # 2^31 / 64: the first stride past 32-bit offsets in a 64-chunk group
# BalancedCfg<4, 2>::kLds: the 4 waves' 2 images of 8 KiB and their 512-B pad are under half a CU's 160 KiB, so the
# workgroup asks for half and 16 KiB more, and a CU runs exactly one
BALANCED_LDS = 160 * 1024 // 2 + 16384
assert 4 * 2 * 8192 + 512 <= 160 * 1024 // 2 < BALANCED_LDS == 98304
MAX_DYN_LDS_ATTR = 8                     # hipFuncAttributeMaxDynamicSharedMemorySize

# enum md5hip_variant, md5hip_desc_variant, crc32hip_variant, md5crc32hip_variant
AUTO = 0
DIRECT2, XDMA1NT = 1, 10
LANE, HYBRID, XDMA, BALANCED, FED, LINES = 1, 3, 4, 5, 6, 7
CRC_XDMA16, CRC_SPLIT = 6, 7
DUAL_XDMA16, DUAL_FEDSPLIT = 1, 2

# The harness's pointers: no kernel runs there, so these are numbers that are
# non-null and aligned as a caller's would be.  The GPU test replaces them.
BASE, OFFS, LENS, ORDER, OUT = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
CTXS, PTRS, NEXT, SEGS, SCRATCH = 0x60000000, 0x70000000, 0x80000000, 0x90000000, 0xA0000000
STREAM = 0x5700
CTR = "CTR"                              # BALANCED's counter: whatever hipMalloc returned


def ceil_div(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------ records
def launch(kernel, grid, block, lds, stream, *args, ns="md5hip::"):
    a = ",".join(x if isinstance(x, str) else hex(x) for x in args)
    return f"launch|{ns}{kernel}|{grid},1,1|{block},1,1|{lds}|{hex(stream)}|{a}"


class Case:
    """One call.  `device`: None gives the call a device of its own (nothing
    cached); cases naming the same device run on one, in table order.
    `shape`: what the GPU test needs to run the same call on real buffers
    (None: the call is not a hash launch, or cannot be run: `why`)."""

    def __init__(self, id, entry, args, rc, records, kernel, shape=None, device=None, why=None):
        self.id, self.entry, self.args, self.rc, self.records = id, entry, list(args), rc, list(records)
        self.kernel, self.shape, self.device, self.why = kernel, shape, device, why

    def line(self, device, cus):
        return " ".join([self.id, str(device), str(cus), self.entry] + [hex(a) for a in self.args])


# ------------------------------------------------------------------ the planner's bounds, from md5hip.h
def fed_fits(groups, cus):
    """'at most one 64-chunk group per CU' (md5hip_plan_desc, md5hip_update_ctx)"""
    return groups <= cus


def per_cu_grid(rows, cus):
    """'one workgroup per CU, grid-stride over 64-row groups'"""
    return min(ceil_div(rows, 64), cus)


def crc_split_grid(n, cus):
    """'4 chunks (waves) per 256-thread workgroup; grid-stride past 8 per CU'"""
    return min(ceil_div(n, 4), 2 * cus)


def crc_split_fits(msgs, length, cus):
    """CRC32HIP_SPLIT: 'up to 128 chunks per CU of >= 2 KiB (12 per CU shorter;
    16 per CU when the lengths are device-side only)'; length 0 = not known"""
    if length == 0:
        return msgs <= 16 * cus
    return msgs <= (128 if length >= 2048 else 12) * cus


def dual_plan(n, length, cus):
    """md5crc32hip_plan: 'FEDSPLIT for at most one 64-chunk group per CU,
    mean_len >= MD5CRC32HIP_FEDSPLIT_MIN_LEN and n <= CUs x mean_len / 256'"""
    ok = n and fed_fits(ceil_div(n, 64), cus) and length >= FEDSPLIT_MIN_LEN and n * 256 <= cus * length
    return DUAL_FEDSPLIT if ok else DUAL_XDMA16


def fedsplit_grid(n, cus):
    """'ceil(n/64) MD5 workgroups, then CRC workgroups of two waves, one chunk
    per wave, at most one per CU'"""
    return ceil_div(n, 64) + min(ceil_div(n, 2), cus)


def on_grid(base, stride):
    return base % 16 == 0 and stride % 16 == 0


# ------------------------------------------------------------------ the routes
# Each returns (rc, records, kernel): kernel None when nothing is launched.
def route_md5_fixed(cus, base, n, length, stride, out, stream, variant):
    if n == 0:
        return 0, [], None
    groups, blocks = ceil_div(n, 64), ceil_div(n, 256)
    lanes = not on_grid(base, stride)                       # 'otherwise the descriptor kernel is used'
    if (not base or not out or length > stride or out % 16 or variant not in (AUTO, DIRECT2, XDMA1NT)
            or (groups if lanes else blocks) > MAXGRID):
        return EINVAL, [], None
    if lanes:
        k = "md5_desc<true>"
        return 0, [launch(k, groups, 64, 0, stream, base, 0, 0, 0, n, stride, length, out)], k
    if variant == DIRECT2 or stride >= FAR:                 # 'used for strides >= 2^31/64'
        k = "md5_fixed_direct"
    elif variant == AUTO and fed_fits(groups, cus) and length >= 128:
        k = "md5_desc_fed<true>"                            # a small batch: fed pairs from two whole blocks on
        return 0, [launch(k, groups, 128, 0, stream, base, 0, 0, 0, n, stride, length, out)], k
    else:
        k = "md5_fixed_xdma1nt"
    return 0, [launch(k, blocks, 256, 0, stream, base, n, length, stride, out)], k


def route_md5_desc(cus, base, offs, lens, order, n, out, stream, variant, first_on_device=True,
                   first_on_stream=True):
    if n == 0:
        return 0, [], None
    groups = ceil_div(n, 64)
    if (not base or not offs or not lens or not out or out % 16
            or variant not in (AUTO, LANE, HYBRID, XDMA, BALANCED, FED, LINES) or groups > MAXGRID):
        return EINVAL, [], None
    a = (base, offs, lens, order, n)
    if variant == HYBRID:                                   # 'the first waves (one per CU) go lane-direct'
        k = "md5_desc_hybrid"
        return 0, [launch(k, groups, 64, 0, stream, *a, out, cus)], k
    if variant == BALANCED:                                 # 'a persistent grid of one wave per SIMD'
        k = "md5_desc_balanced_t<4, 2, 2>"
        pre = []
        if first_on_stream:                                 # one counter set per (device, stream), zeroed at birth
            pre += [f"malloc|{CTR}|16", f"memset|{CTR}|0|16"]
        if first_on_device:                                 # the dynamic-LDS limit, raised once per device
            pre += [f"attr|md5hip::{k}|{MAX_DYN_LDS_ATTR}|{BALANCED_LDS}"]
        pre += [f"memset_async|{CTR}|0|16|{hex(stream)}"]   # 'zero it on the stream anyway'
        return 0, pre + [launch(k, cus, 256, BALANCED_LDS, stream, *a, out, CTR)], k
    if variant == FED:
        k = "md5_desc_fed<false>"
        return 0, [launch(k, groups, 128, 0, stream, *a, 0, 0, out)], k
    if variant == LANE:
        k = "md5_desc<false>"
        return 0, [launch(k, groups, 64, 0, stream, *a, 0, 0, out)], k
    k = "md5_desc_lines" if variant == LINES else "md5_desc_xdma"      # AUTO: 'the default: XDMA'
    return 0, [launch(k, groups, 64, 0, stream, *a, out)], k


def crc_ladder(cus, base, offs, lens, order, n, stride, flen, fastcrc, windows, split_len, variant, out, stream):
    """The part both CRC entries share; None when whole chunks do not split."""
    split = variant == CRC_SPLIT or (variant == AUTO and crc_split_fits(2 * n if windows else n, split_len, cus))
    if (not windows or fastcrc >= 2048) and split:          # 'fastcrc windows of >= 2 KiB split as two messages'
        k = "crc32_split<false>" if offs else "crc32_split<true>"
        return 0, [launch(k, crc_split_grid(n, cus), 256, 0, stream, base, offs, lens, order, n, stride, flen,
                          fastcrc, out)], k
    if not windows:
        return None
    pipe = fastcrc in (64, 128)                             # one- or two-block windows
    k = "crc32_fast_pipe" if pipe else "crc32_fast_xdma16"
    return 0, [launch(k, per_cu_grid(2 * n, cus), 1024 if pipe else 768, 0, stream, base, offs, lens, n, stride,
                      flen, fastcrc, out)], k


def route_crc_fixed(cus, base, n, length, stride, fastcrc, out, stream, variant):
    if n == 0:
        return 0, [], None
    groups = ceil_div(n, 64)
    if (not base or not out or length > stride or fastcrc % 4 or out % 4
            or variant not in (AUTO, CRC_XDMA16, CRC_SPLIT) or groups > MAXGRID):
        return EINVAL, [], None
    windows = fastcrc != 0 and length > fastcrc             # 'fastcrc == 0 || len_i <= fastcrc ? crc32(chunk_i)'
    r = crc_ladder(cus, base, 0, 0, 0, n, stride, length, fastcrc, windows,
                   fastcrc if windows else max(length, 1), variant, out, stream)
    if r:
        return r
    if on_grid(base, stride) and stride < FAR:
        k = "crc32_fixed_xdma16"
        return 0, [launch(k, per_cu_grid(n, cus), 768, 0, stream, base, n, length, stride, out)], k
    k = "crc32_desc<true>"
    return 0, [launch(k, groups, 64, 0, stream, base, 0, 0, 0, n, stride, length, out)], k


def route_crc_desc(cus, base, offs, lens, order, n, fastcrc, out, stream, variant):
    if n == 0:
        return 0, [], None
    if (not base or not offs or not lens or not out or fastcrc % 4 or out % 4
            or variant not in (AUTO, CRC_XDMA16, CRC_SPLIT) or ceil_div(n, 64) > MAXGRID):
        return EINVAL, [], None
    # the lengths are on the device: windows whenever fastcrc is set, no length for the split decision
    r = crc_ladder(cus, base, offs, lens, order, n, 0, 0, fastcrc, fastcrc != 0, 0, variant, out, stream)
    if r:
        return r
    k = "crc32_desc_xdma16"
    return 0, [launch(k, per_cu_grid(n, cus), 768, 0, stream, base, offs, lens, order, n, out)], k


def route_dual_fixed(cus, base, n, length, stride, out, stream, variant=None):
    """variant None: the plain entry, which 'launches XDMA16 for every batch'"""
    if n == 0:
        return 0, [], None
    grid = ceil_div(n, 64) if variant is None else fedsplit_grid(n, cus)
    if (not base or not out or length > stride or out % 16
            or variant not in (None, AUTO, DUAL_XDMA16, DUAL_FEDSPLIT) or grid > MAXGRID):
        return EINVAL, [], None
    fast = on_grid(base, stride) and stride < FAR
    if variant == AUTO:                                     # 'FEDSPLIT only from a 16-B aligned base and stride below 2^31/64'
        variant = dual_plan(n, length, cus) if fast else DUAL_XDMA16
    if variant == DUAL_FEDSPLIT:                            # 'any n, alignment and stride'
        k = "md5crc32_fedsplit<true>"
        return 0, [launch(k, fedsplit_grid(n, cus), 128, 0, stream, base, 0, 0, 0, n, stride, length, out)], k
    if fast:
        k = "md5crc32_fixed_xdma16"
        return 0, [launch(k, per_cu_grid(n, cus), 768, 0, stream, base, n, length, stride, out)], k
    k = "md5crc32_desc_xdma16<true>"
    return 0, [launch(k, per_cu_grid(n, cus), 768, 0, stream, base, 0, 0, 0, n, stride, length, out)], k


def route_dual_desc(cus, base, offs, lens, order, n, out, stream, variant=None):
    if n == 0:
        return 0, [], None
    grid = ceil_div(n, 64) if variant is None else fedsplit_grid(n, cus)
    if (not base or not offs or not lens or not out or out % 16
            or variant not in (None, AUTO, DUAL_XDMA16, DUAL_FEDSPLIT) or grid > MAXGRID):
        return EINVAL, [], None
    if variant == DUAL_FEDSPLIT:                            # AUTO of the desc entry 'is XDMA16'
        k = "md5crc32_fedsplit<false>"
        return 0, [launch(k, fedsplit_grid(n, cus), 128, 0, stream, base, offs, lens, order, n, 0, 0, out)], k
    k = "md5crc32_desc_xdma16<false>"
    return 0, [launch(k, per_cu_grid(n, cus), 768, 0, stream, base, offs, lens, order, n, 0, 0, out)], k


def route_update_ctx(cus, ctxs, ptrs, lens, n, stream):
    if n == 0:
        return 0, [], None
    groups = ceil_div(n, 64)                                # one wave per 64 contexts
    if not ctxs or not ptrs or not lens or ctxs % 4 or groups > MAXGRID:
        return EINVAL, [], None
    fed = fed_fits(groups, cus)                             # 'at most 64 contexts per CU ... as fed pairs'
    k = "md5_update_ctx_fed" if fed else "md5_update_ctx"
    return 0, [launch(k, groups, 128 if fed else 64, 0, stream, ctxs, ptrs, lens, n)], k


def route_blocks_of_256(kernel, n, ok, stream, *args):
    """init_ctx, final_ctx, order_device: one thread per item, 256 per workgroup"""
    if n == 0:
        return 0, [], None
    if not ok or ceil_div(n, 256) > MAXGRID:
        return EINVAL, [], None
    return 0, [launch(kernel, ceil_div(n, 256), 256, 0, stream, *args)], kernel


# ---- page lists (md5_pages.hip).  Its kernels live in an unnamed namespace, and the records drop that
# prefix (fake_hip_rt.cc), so their names carry no "md5hip::"; a PageBatch argument is recorded as its
# five fields: pages, first, lens, order, page_bytes.
DIGEST_MD5, DIGEST_CRC32, DIGEST_DUAL = 0, 1, 2              # enum md5hip_digest_kind
PAGE_BYTES_MAX = 1 << 30                                     # MD5HIP_PAGE_BYTES_MAX
PAGES_MD5, PAGES_CTX, PAGES_FAST = "md5_pages_xdma", "md5_update_ctx_pages", "crc32_pages_fast"
PAGES_CRC, PAGES_DUAL = "pages_xdma16<md5hip::Crc32PermHasher>", "pages_xdma16<md5hip::Md5Crc32Hasher>"
PAGED_KERNELS = (PAGES_MD5, PAGES_CRC, PAGES_DUAL, PAGES_FAST, PAGES_CTX)


def page_bytes_ok(page_bytes):
    """'page_bytes is a multiple of 128, at most MD5HIP_PAGE_BYTES_MAX'"""
    return page_bytes != 0 and page_bytes % 128 == 0 and page_bytes <= PAGE_BYTES_MAX


def route_digest_pages(cus, kind, pages, first, lens, order, n, page_bytes, out, stream):
    if n == 0:                                              # 'n == 0: a no-op returning 0'
        return 0, [], None
    align = {DIGEST_MD5: 16, DIGEST_CRC32: 4, DIGEST_DUAL: 16}.get(kind)   # 'aligned to 16, 4 and 16'
    groups = ceil_div(n, 64)
    if (align is None or not pages or not first or not lens or not out or out % align
            or not page_bytes_ok(page_bytes) or groups > MAXGRID):
        return EINVAL, [], None
    pb = (pages, first, lens, order, page_bytes)
    if kind == DIGEST_MD5:                                  # one wave per workgroup, as md5_desc_xdma
        return 0, [launch(PAGES_MD5, groups, 64, 0, stream, *pb, n, out, ns="")], PAGES_MD5
    k = PAGES_CRC if kind == DIGEST_CRC32 else PAGES_DUAL   # 'one 768-thread workgroup per CU, grid-stride'
    return 0, [launch(k, per_cu_grid(n, cus), 768, 0, stream, *pb, n, out, ns="")], k


def route_crc_pages(cus, pages, first, lens, order, n, page_bytes, fastcrc, out, stream):
    if fastcrc == 0:                                        # 'fastcrc == 0 IS md5hip_digest_pages(MD5HIP_DIGEST_CRC32, ..)'
        return route_digest_pages(cus, DIGEST_CRC32, pages, first, lens, order, n, page_bytes, out, stream)
    if n == 0:
        return 0, [], None
    groups = ceil_div(n, 32)                                # 64 window rows each
    if (not pages or not first or not lens or not out or out % 4 or fastcrc % 4 or not page_bytes_ok(page_bytes)
            or groups > MAXGRID):
        return EINVAL, [], None
    # 'every window has the same length, so d_order is not read': the kernel never gets it
    return 0, [launch(PAGES_FAST, min(groups, cus), 1024, 0, stream, pages, first, lens, 0, page_bytes, n, fastcrc,
                      out, ns="")], PAGES_FAST


def route_update_ctx_pages(cus, ctxs, pages, first, lens, n, page_bytes, stream):
    if n == 0:
        return 0, [], None
    groups = ceil_div(n, 64)                                # one wave per 64 contexts; 'There is no d_order'
    if (not ctxs or not pages or not first or not lens or ctxs % 4 or not page_bytes_ok(page_bytes)
            or groups > MAXGRID):
        return EINVAL, [], None
    return 0, [launch(PAGES_CTX, groups, 64, 0, stream, ctxs, pages, first, lens, 0, page_bytes, n, ns="")], PAGES_CTX


# ------------------------------------------------------------------ the table
def cases(cus):
    out, seen = [], set()

    def add(id, entry, args, route, kernel, shape=None, device=None, why=None):
        rc, records, k = route
        want = {None: None, EINVAL: None}.get(kernel, kernel)
        assert k == want, f"{id} at {cus} CUs: the table says {kernel}, its route {k}"
        assert rc == (EINVAL if kernel == EINVAL else 0), f"{id} at {cus} CUs: rc {rc}"
        assert id not in seen, id
        seen.add(id)
        out.append(Case(id, entry, args, rc, records, k, shape if rc == 0 and k else None, device, why))

    HUGE = "a grid of 2^31 - 1 workgroups: more chunks than a device holds"

    # ---- fixed-length MD5
    def md5_fixed(id, n, length, stride, kernel, base=BASE, out_=OUT, variant=None, stream=STREAM, why=None):
        v = AUTO if variant is None else variant
        route = route_md5_fixed(cus, base, n, length, stride, out_, stream, v)
        entry = "md5hip_digest_fixed" if variant is None else "md5hip_digest_fixed_variant"
        args = [base, n, length, stride, out_, stream] + ([] if variant is None else [variant])
        shape = None if why else dict(kind="md5_fixed", skew=base - BASE, n=n, len=length, stride=stride,
                                      variant=variant)
        add("md5_fixed." + id, entry, args, route, kernel, shape, why=why)

    md5_fixed("empty", 0, 128, 128, None, base=0, out_=0)
    md5_fixed("null_base", 64, 128, 128, EINVAL, base=0)
    md5_fixed("null_out", 64, 128, 128, EINVAL, out_=0)
    md5_fixed("len_past_stride", 64, 129, 128, EINVAL)
    md5_fixed("out_off_16", 64, 128, 128, EINVAL, out_=OUT + 8)
    md5_fixed("variant_2", 64, 128, 128, EINVAL, variant=2)
    md5_fixed("variant_11", 64, 128, 128, EINVAL, variant=11)
    md5_fixed("grid_limit", 256 * MAXGRID, 64, 64, "md5_fixed_xdma1nt", why=HUGE)
    md5_fixed("grid_limit_plus_1", 256 * MAXGRID + 1, 64, 64, EINVAL)
    md5_fixed("grid_limit_off_16", 64 * MAXGRID, 64, 64, "md5_desc<true>", base=BASE + 8, why=HUGE)
    md5_fixed("grid_limit_off_16_plus_1", 64 * MAXGRID + 1, 64, 64, EINVAL, base=BASE + 8)
    md5_fixed("base_off_16", 100, 2048, 2048, "md5_desc<true>", base=BASE + 8)
    md5_fixed("base_on_16", 100, 2048, 2048, "md5_desc_fed<true>", base=BASE + 16)
    md5_fixed("stride_off_16", 100, 2048, 2056, "md5_desc<true>")
    md5_fixed("stride_on_16", 100, 2048, 2064, "md5_desc_fed<true>")
    md5_fixed("stride_below_far", 2, 128, FAR - 16, "md5_desc_fed<true>")
    md5_fixed("stride_far", 2, 128, FAR, "md5_fixed_direct")
    md5_fixed("xdma1nt_stride_below_far", 2, 128, FAR - 16, "md5_fixed_xdma1nt", variant=XDMA1NT)
    md5_fixed("xdma1nt_stride_far", 2, 128, FAR, "md5_fixed_direct", variant=XDMA1NT)
    md5_fixed("groups_at_cus", 64 * cus, 128, 128, "md5_desc_fed<true>")
    md5_fixed("groups_past_cus", 64 * cus + 1, 128, 128, "md5_fixed_xdma1nt")
    md5_fixed("len_127", 64, 127, 128, "md5_fixed_xdma1nt")
    md5_fixed("len_128", 64, 128, 128, "md5_desc_fed<true>")
    md5_fixed("auto_16k", 64, 16384, 16384, "md5_desc_fed<true>", variant=AUTO)
    md5_fixed("xdma1nt_named", 64, 16384, 16384, "md5_fixed_xdma1nt", variant=XDMA1NT)   # never the fed kernel
    md5_fixed("direct2_named", 64, 16384, 16384, "md5_fixed_direct", variant=DIRECT2)
    md5_fixed("direct2_off_16", 64, 300, 301, "md5_desc<true>", variant=DIRECT2)
    md5_fixed("null_stream", 300, 64, 64, "md5_fixed_xdma1nt", stream=0)

    # ---- descriptor MD5
    def md5_desc(id, n, kernel, variant=None, base=BASE, offs=OFFS, lens=LENS, order=ORDER, out_=OUT, why=None,
                 device=None, stream=STREAM, **first):
        v = AUTO if variant is None else variant
        route = route_md5_desc(cus, base, offs, lens, order, n, out_, stream, v, **first)
        entry = "md5hip_digest_desc" if variant is None else "md5hip_digest_desc_variant"
        args = [base, offs, lens, order, n, out_, stream] + ([] if variant is None else [variant])
        shape = None if why else dict(kind="md5_desc", n=n, len=2048, order=bool(order), variant=variant)
        add("md5_desc." + id, entry, args, route, kernel, shape, device=device, why=why)

    md5_desc("empty", 0, None, base=0, offs=0, lens=0, out_=0)
    md5_desc("null_base", 100, EINVAL, base=0)
    md5_desc("null_offsets", 100, EINVAL, offs=0)
    md5_desc("null_lens", 100, EINVAL, lens=0)
    md5_desc("null_out", 100, EINVAL, out_=0)
    md5_desc("out_off_16", 100, EINVAL, out_=OUT + 4)
    md5_desc("variant_2", 100, EINVAL, variant=2)
    md5_desc("variant_8", 100, EINVAL, variant=8)
    md5_desc("grid_limit", 64 * MAXGRID, "md5_desc_xdma", why=HUGE)
    md5_desc("grid_limit_plus_1", 64 * MAXGRID + 1, EINVAL)
    md5_desc("no_order", 1000, "md5_desc_xdma", order=0)
    md5_desc("plain", 1000, "md5_desc_xdma")
    md5_desc("auto", 65, "md5_desc_xdma", variant=AUTO)
    md5_desc("lane", 1000, "md5_desc<false>", variant=LANE)
    md5_desc("hybrid", 1000, "md5_desc_hybrid", variant=HYBRID)                 # nlong = CUs
    md5_desc("xdma", 1000, "md5_desc_xdma", variant=XDMA)
    md5_desc("fed", 1000, "md5_desc_fed<false>", variant=FED)
    md5_desc("fed_past_cus", 64 * cus + 1, "md5_desc_fed<false>", variant=FED)  # named: the planner's bound is not the launcher's
    md5_desc("lines", 1000, "md5_desc_lines", variant=LINES)
    md5_desc("balanced", 1000, "md5_desc_balanced_t<4, 2, 2>", variant=BALANCED)
    md5_desc("balanced_one_chunk", 1, "md5_desc_balanced_t<4, 2, 2>", variant=BALANCED)   # the grid is CUs all the same
    md5_desc("balanced_first", 1000, "md5_desc_balanced_t<4, 2, 2>", variant=BALANCED, device="balanced")
    md5_desc("balanced_again", 130, "md5_desc_balanced_t<4, 2, 2>", variant=BALANCED, device="balanced",
             first_on_device=False, first_on_stream=False)
    md5_desc("balanced_other_stream", 130, "md5_desc_balanced_t<4, 2, 2>", variant=BALANCED, device="balanced",
             stream=STREAM + 0x100, first_on_device=False)

    # ---- fixed-length CRC-32
    def crc_fixed(id, n, length, stride, fastcrc, kernel, base=BASE, out_=OUT, variant=None, why=None):
        v = AUTO if variant is None else variant
        route = route_crc_fixed(cus, base, n, length, stride, fastcrc, out_, STREAM, v)
        entry = "crc32hip_fixed" if variant is None else "crc32hip_fixed_variant"
        args = [base, n, length, stride, fastcrc, out_, STREAM] + ([] if variant is None else [variant])
        shape = None if why else dict(kind="crc_fixed", skew=base - BASE, n=n, len=length, stride=stride,
                                      fastcrc=fastcrc, variant=variant)
        add("crc_fixed." + id, entry, args, route, kernel, shape, why=why)

    crc_fixed("empty", 0, 128, 128, 0, None, base=0, out_=0)
    crc_fixed("null_base", 64, 128, 128, 0, EINVAL, base=0)
    crc_fixed("null_out", 64, 128, 128, 0, EINVAL, out_=0)
    crc_fixed("len_past_stride", 64, 129, 128, 0, EINVAL)
    crc_fixed("fastcrc_6", 64, 128, 128, 6, EINVAL)
    crc_fixed("out_off_4", 64, 128, 128, 0, EINVAL, out_=OUT + 2)
    crc_fixed("variant_1", 64, 128, 128, 0, EINVAL, variant=1)
    crc_fixed("variant_8", 64, 128, 128, 0, EINVAL, variant=8)
    crc_fixed("grid_limit", 64 * MAXGRID, 64, 64, 0, "crc32_fixed_xdma16", why=HUGE)
    crc_fixed("grid_limit_plus_1", 64 * MAXGRID + 1, 64, 64, 0, EINVAL)
    # whole chunks: 128 per CU from 2 KiB on, 12 per CU below, a length of 0 counted as short
    crc_fixed("2k_at_128_per_cu", 128 * cus, 2048, 2048, 0, "crc32_split<true>")
    crc_fixed("2k_past_128_per_cu", 128 * cus + 1, 2048, 2048, 0, "crc32_fixed_xdma16")
    crc_fixed("short_at_12_per_cu", 12 * cus, 2047, 2048, 0, "crc32_split<true>")
    crc_fixed("short_past_12_per_cu", 12 * cus + 1, 2047, 2048, 0, "crc32_fixed_xdma16")
    crc_fixed("len_0_at_12_per_cu", 12 * cus, 0, 16, 0, "crc32_split<true>")
    crc_fixed("len_0_past_12_per_cu", 12 * cus + 1, 0, 16, 0, "crc32_fixed_xdma16")
    # crc_split_grid: ceil(n / 4), at most two workgroups per CU
    crc_fixed("split_grid_under_cap", 8 * cus - 4, 2048, 2048, 0, "crc32_split<true>")
    crc_fixed("split_grid_at_cap", 8 * cus, 2048, 2048, 0, "crc32_split<true>")
    crc_fixed("split_grid_capped", 8 * cus + 1, 2048, 2048, 0, "crc32_split<true>")
    crc_fixed("split_named_past_128_per_cu", 128 * cus + 1, 2048, 2048, 0, "crc32_split<true>", variant=CRC_SPLIT)
    # per_cu_grid over n rows
    crc_fixed("xdma16_named_small", 4, 2048, 2048, 0, "crc32_fixed_xdma16", variant=CRC_XDMA16)
    crc_fixed("xdma16_grid_under_cap", 64 * cus - 64, 256, 256, 0, "crc32_fixed_xdma16", variant=CRC_XDMA16)
    crc_fixed("xdma16_grid_at_cap", 64 * cus, 256, 256, 0, "crc32_fixed_xdma16", variant=CRC_XDMA16)
    crc_fixed("xdma16_grid_capped", 64 * cus + 1, 256, 256, 0, "crc32_fixed_xdma16", variant=CRC_XDMA16)
    # whole chunks off the fixed loader's ground
    crc_fixed("base_off_16", 200, 256, 256, 0, "crc32_desc<true>", base=BASE + 4, variant=CRC_XDMA16)
    crc_fixed("stride_off_16", 200, 256, 264, 0, "crc32_desc<true>", variant=CRC_XDMA16)
    crc_fixed("stride_below_far", 2, 256, FAR - 16, 0, "crc32_fixed_xdma16", variant=CRC_XDMA16)
    crc_fixed("stride_far", 2, 256, FAR, 0, "crc32_desc<true>", variant=CRC_XDMA16)
    crc_fixed("split_off_16", 200, 2048, 2049, 0, "crc32_split<true>", base=BASE + 1)
    # a window no shorter than the chunk: whole chunks
    crc_fixed("window_of_len", 4, 4096, 4096, 4096, "crc32_split<true>")
    crc_fixed("window_4096_of_4100", 4, 4100, 4112, 4096, "crc32_split<true>")
    crc_fixed("window_of_len_xdma16", 4, 4096, 4096, 4096, "crc32_fixed_xdma16", variant=CRC_XDMA16)
    # windows by size: F = 64 and 128 pipe, under 2 KiB the window loader, from 2 KiB on split
    for F, k in ((4, "crc32_fast_xdma16"), (64, "crc32_fast_pipe"), (128, "crc32_fast_pipe"),
                 (1000, "crc32_fast_xdma16"), (2044, "crc32_fast_xdma16"), (2048, "crc32_split<true>")):
        crc_fixed(f"window_{F}", 100, 8192, 8192, F, k)
    crc_fixed("split_named_window_1000", 100, 8192, 8192, 1000, "crc32_fast_xdma16", variant=CRC_SPLIT)
    crc_fixed("split_named_window_64", 100, 8192, 8192, 64, "crc32_fast_pipe", variant=CRC_SPLIT)
    crc_fixed("split_named_window_2048", 128 * cus, 4096, 4096, 2048, "crc32_split<true>", variant=CRC_SPLIT)
    crc_fixed("xdma16_named_window_2048", 100, 8192, 8192, 2048, "crc32_fast_xdma16", variant=CRC_XDMA16)
    # two windows per chunk count as two messages: 2n against 128 per CU
    crc_fixed("window_2048_at_128_per_cu", 64 * cus, 4096, 4096, 2048, "crc32_split<true>")
    crc_fixed("window_2048_past_128_per_cu", 64 * cus + 1, 4096, 4096, 2048, "crc32_fast_xdma16")
    # per_cu_grid over 2n rows
    crc_fixed("window_rows_33", 33, 256, 256, 64, "crc32_fast_pipe")
    crc_fixed("window_rows_under_cap", 32 * cus - 32, 256, 256, 64, "crc32_fast_pipe")
    crc_fixed("window_rows_at_cap", 32 * cus, 256, 256, 64, "crc32_fast_pipe")
    crc_fixed("window_rows_capped", 32 * cus + 1, 256, 256, 128, "crc32_fast_pipe")
    crc_fixed("window_rows_capped_xdma16", 32 * cus + 1, 2048, 2048, 1000, "crc32_fast_xdma16")

    # ---- descriptor CRC-32 (lengths on the device: 16 per CU)
    def crc_desc(id, n, fastcrc, kernel, variant=None, base=BASE, offs=OFFS, lens=LENS, order=ORDER, out_=OUT,
                 why=None, length=2048):
        v = AUTO if variant is None else variant
        route = route_crc_desc(cus, base, offs, lens, order, n, fastcrc, out_, STREAM, v)
        entry = "crc32hip_desc" if variant is None else "crc32hip_desc_variant"
        args = [base, offs, lens, order, n, fastcrc, out_, STREAM] + ([] if variant is None else [variant])
        shape = None if why else dict(kind="crc_desc", n=n, len=length, order=bool(order), fastcrc=fastcrc,
                                      variant=variant)
        add("crc_desc." + id, entry, args, route, kernel, shape, why=why)

    crc_desc("empty", 0, 0, None, base=0, offs=0, lens=0, out_=0)
    crc_desc("null_base", 100, 0, EINVAL, base=0)
    crc_desc("null_offsets", 100, 0, EINVAL, offs=0)
    crc_desc("null_lens", 100, 0, EINVAL, lens=0)
    crc_desc("null_out", 100, 0, EINVAL, out_=0)
    crc_desc("fastcrc_2", 100, 2, EINVAL)
    crc_desc("out_off_4", 100, 0, EINVAL, out_=OUT + 1)
    crc_desc("variant_5", 100, 0, EINVAL, variant=5)
    crc_desc("grid_limit", 64 * MAXGRID, 0, "crc32_desc_xdma16", why=HUGE)
    crc_desc("grid_limit_plus_1", 64 * MAXGRID + 1, 0, EINVAL)
    crc_desc("at_16_per_cu", 16 * cus, 0, "crc32_split<false>", length=300)
    crc_desc("past_16_per_cu", 16 * cus + 1, 0, "crc32_desc_xdma16", length=300)
    crc_desc("no_order", 100, 0, "crc32_split<false>", order=0)
    crc_desc("window_2048_at_16_per_cu", 8 * cus, 2048, "crc32_split<false>", length=4500)
    crc_desc("window_2048_past_16_per_cu", 8 * cus + 1, 2048, "crc32_fast_xdma16", length=4500)
    crc_desc("window_64", 100, 64, "crc32_fast_pipe", length=300)
    crc_desc("window_128", 100, 128, "crc32_fast_pipe", length=300)
    crc_desc("window_2044", 100, 2044, "crc32_fast_xdma16", length=4500)
    crc_desc("split_named_window_1000", 100, 1000, "crc32_fast_xdma16", variant=CRC_SPLIT, length=4500)
    crc_desc("split_named_past_16_per_cu", 16 * cus + 1, 0, "crc32_split<false>", variant=CRC_SPLIT, length=300)
    crc_desc("xdma16_named_small", 100, 0, "crc32_desc_xdma16", variant=CRC_XDMA16)
    crc_desc("xdma16_grid_capped", 64 * cus + 1, 0, "crc32_desc_xdma16", variant=CRC_XDMA16, length=300)
    crc_desc("xdma16_named_window_4096", 100, 4096, "crc32_fast_xdma16", variant=CRC_XDMA16, length=9000)

    # ---- MD5 + CRC-32 in one pass, fixed length
    def dual_fixed(id, n, length, stride, kernel, base=BASE, out_=OUT, variant=None, why=None):
        route = route_dual_fixed(cus, base, n, length, stride, out_, STREAM, variant)
        entry = "md5crc32hip_fixed" if variant is None else "md5crc32hip_fixed_variant"
        args = [base, n, length, stride, out_, STREAM] + ([] if variant is None else [variant])
        shape = None if why else dict(kind="dual_fixed", skew=base - BASE, n=n, len=length, stride=stride,
                                      variant=variant)
        add("dual_fixed." + id, entry, args, route, kernel, shape, why=why)

    dual_fixed("empty", 0, 128, 128, None, base=0, out_=0)
    dual_fixed("null_base", 64, 128, 128, EINVAL, base=0)
    dual_fixed("null_out", 64, 128, 128, EINVAL, out_=0)
    dual_fixed("len_past_stride", 64, 129, 128, EINVAL)
    dual_fixed("out_off_16", 64, 128, 128, EINVAL, out_=OUT + 8)
    dual_fixed("grid_limit", 64 * MAXGRID, 64, 64, "md5crc32_fixed_xdma16", why=HUGE)
    dual_fixed("grid_limit_plus_1", 64 * MAXGRID + 1, 64, 64, EINVAL)
    dual_fixed("on_16", 300, 2048, 2048, "md5crc32_fixed_xdma16")
    dual_fixed("base_off_16", 300, 2048, 2048, "md5crc32_desc_xdma16<true>", base=BASE + 8)
    dual_fixed("stride_off_16", 300, 2048, 2052, "md5crc32_desc_xdma16<true>")
    dual_fixed("stride_below_far", 2, 2048, FAR - 16, "md5crc32_fixed_xdma16")
    dual_fixed("stride_far", 2, 2048, FAR, "md5crc32_desc_xdma16<true>")
    dual_fixed("grid_at_cap", 64 * cus, 128, 128, "md5crc32_fixed_xdma16")
    dual_fixed("grid_capped", 64 * cus + 1, 128, 128, "md5crc32_fixed_xdma16")
    dual_fixed("grid_capped_off_16", 64 * cus + 1, 120, 120, "md5crc32_desc_xdma16<true>")
    # the entry that names the kernel
    dual_fixed("empty_variant", 0, 128, 128, None, variant=DUAL_FEDSPLIT, base=0, out_=0)
    dual_fixed("variant_3", 64, 128, 128, EINVAL, variant=3)
    dual_fixed("variant_minus_1", 64, 128, 128, EINVAL, variant=2**32 - 1)
    dual_fixed("variant_null_out", 64, 128, 128, EINVAL, variant=AUTO, out_=0)
    dual_fixed("variant_len_past_stride", 64, 129, 128, EINVAL, variant=DUAL_FEDSPLIT)
    dual_fixed("fedsplit_grid_limit", 64 * (MAXGRID - cus), 64, 64, "md5crc32_fedsplit<true>",
               variant=DUAL_FEDSPLIT, why=HUGE)
    dual_fixed("fedsplit_grid_limit_plus_1", 64 * (MAXGRID - cus) + 1, 64, 64, EINVAL, variant=DUAL_FEDSPLIT)
    # AUTO: n x 256 <= CUs x len, the length from MD5CRC32HIP_FEDSPLIT_MIN_LEN, one group per CU
    dual_fixed("auto_count_at_bound", 4 * cus, 1024, 1024, "md5crc32_fedsplit<true>", variant=AUTO)
    dual_fixed("auto_count_past_bound", 4 * cus + 1, 1024, 1024, "md5crc32_fixed_xdma16", variant=AUTO)
    dual_fixed("auto_min_len", cus, 1024, 1024, "md5crc32_fedsplit<true>", variant=AUTO)
    dual_fixed("auto_under_min_len", cus, 1023, 1024, "md5crc32_fixed_xdma16", variant=AUTO)
    dual_fixed("auto_groups_at_cus", 64 * cus, 16384, 16384, "md5crc32_fedsplit<true>", variant=AUTO)
    dual_fixed("auto_groups_past_cus", 64 * cus + 1, 16384, 16384, "md5crc32_fixed_xdma16", variant=AUTO)
    # AUTO withheld from chunk starts off the 16-B grid and from far strides
    dual_fixed("auto_base_off_16", cus, 1024, 1024, "md5crc32_desc_xdma16<true>", variant=AUTO, base=BASE + 8)
    dual_fixed("auto_stride_off_16", cus, 1024, 1032, "md5crc32_desc_xdma16<true>", variant=AUTO)
    dual_fixed("auto_stride_below_far", 2, 1024, FAR - 16, "md5crc32_fedsplit<true>", variant=AUTO)
    dual_fixed("auto_stride_far", 2, 1024, FAR, "md5crc32_desc_xdma16<true>", variant=AUTO)
    # FEDSPLIT named: any n, alignment and stride; fedsplit_grid = ceil(n / 64) + min(ceil(n / 2), CUs)
    dual_fixed("fedsplit_one_chunk", 1, 300, 304, "md5crc32_fedsplit<true>", variant=DUAL_FEDSPLIT)
    dual_fixed("fedsplit_base_off_16", 100, 300, 301, "md5crc32_fedsplit<true>", variant=DUAL_FEDSPLIT, base=BASE + 3)
    dual_fixed("fedsplit_stride_far", 2, 1024, FAR, "md5crc32_fedsplit<true>", variant=DUAL_FEDSPLIT)
    dual_fixed("fedsplit_half_cus", cus, 256, 256, "md5crc32_fedsplit<true>", variant=DUAL_FEDSPLIT)
    dual_fixed("fedsplit_crc_under_cap", 2 * cus - 2, 256, 256, "md5crc32_fedsplit<true>", variant=DUAL_FEDSPLIT)
    dual_fixed("fedsplit_crc_at_cap", 2 * cus, 256, 256, "md5crc32_fedsplit<true>", variant=DUAL_FEDSPLIT)
    dual_fixed("fedsplit_crc_capped", 2 * cus + 1, 256, 256, "md5crc32_fedsplit<true>", variant=DUAL_FEDSPLIT)
    dual_fixed("fedsplit_past_cus_groups", 64 * cus + 1, 128, 128, "md5crc32_fedsplit<true>", variant=DUAL_FEDSPLIT)
    dual_fixed("xdma16_named_small", 64, 16384, 16384, "md5crc32_fixed_xdma16", variant=DUAL_XDMA16)

    # ---- MD5 + CRC-32 in one pass, descriptors
    def dual_desc(id, n, kernel, variant=None, base=BASE, offs=OFFS, lens=LENS, order=ORDER, out_=OUT, why=None):
        route = route_dual_desc(cus, base, offs, lens, order, n, out_, STREAM, variant)
        entry = "md5crc32hip_desc" if variant is None else "md5crc32hip_desc_variant"
        args = [base, offs, lens, order, n, out_, STREAM] + ([] if variant is None else [variant])
        shape = None if why else dict(kind="dual_desc", n=n, len=2048, order=bool(order), variant=variant)
        add("dual_desc." + id, entry, args, route, kernel, shape, why=why)

    dual_desc("empty", 0, None, base=0, offs=0, lens=0, out_=0)
    dual_desc("null_base", 100, EINVAL, base=0)
    dual_desc("null_offsets", 100, EINVAL, offs=0)
    dual_desc("null_lens", 100, EINVAL, lens=0)
    dual_desc("null_out", 100, EINVAL, out_=0)
    dual_desc("out_off_16", 100, EINVAL, out_=OUT + 8)
    dual_desc("grid_limit", 64 * MAXGRID, "md5crc32_desc_xdma16<false>", why=HUGE)
    dual_desc("grid_limit_plus_1", 64 * MAXGRID + 1, EINVAL)
    dual_desc("plain", 300, "md5crc32_desc_xdma16<false>")
    dual_desc("no_order", 300, "md5crc32_desc_xdma16<false>", order=0)
    dual_desc("grid_capped", 64 * cus + 1, "md5crc32_desc_xdma16<false>")
    dual_desc("variant_3", 100, EINVAL, variant=3)
    dual_desc("variant_null_lens", 100, EINVAL, variant=DUAL_FEDSPLIT, lens=0)
    dual_desc("fedsplit_grid_limit_plus_1", 64 * (MAXGRID - cus) + 1, EINVAL, variant=DUAL_XDMA16)
    dual_desc("auto_small", 64, "md5crc32_desc_xdma16<false>", variant=AUTO)    # the lengths are on the device
    dual_desc("xdma16_named", 64, "md5crc32_desc_xdma16<false>", variant=DUAL_XDMA16)
    dual_desc("fedsplit", 300, "md5crc32_fedsplit<false>", variant=DUAL_FEDSPLIT)
    dual_desc("fedsplit_no_order", 65, "md5crc32_fedsplit<false>", variant=DUAL_FEDSPLIT, order=0)
    dual_desc("fedsplit_crc_capped", 2 * cus + 1, "md5crc32_fedsplit<false>", variant=DUAL_FEDSPLIT)

    # ---- batched MD5Init / MD5Update / MD5Final
    def update_ctx(id, n, kernel, ctxs=CTXS, ptrs=PTRS, lens=LENS, why=None):
        route = route_update_ctx(cus, ctxs, ptrs, lens, n, STREAM)
        shape = None if why else dict(kind="update_ctx", n=n, len=200)
        add("update_ctx." + id, "md5hip_update_ctx", [ctxs, ptrs, lens, n, STREAM], route, kernel, shape, why=why)

    update_ctx("empty", 0, None, ctxs=0, ptrs=0, lens=0)
    update_ctx("null_ctxs", 64, EINVAL, ctxs=0)
    update_ctx("null_ptrs", 64, EINVAL, ptrs=0)
    update_ctx("null_lens", 64, EINVAL, lens=0)
    update_ctx("ctxs_off_4", 64, EINVAL, ctxs=CTXS + 2)
    update_ctx("grid_limit", 64 * MAXGRID, "md5_update_ctx", why=HUGE)
    update_ctx("grid_limit_plus_1", 64 * MAXGRID + 1, EINVAL)
    update_ctx("one", 1, "md5_update_ctx_fed")
    update_ctx("groups_at_cus", 64 * cus, "md5_update_ctx_fed")
    update_ctx("groups_past_cus", 64 * cus + 1, "md5_update_ctx")

    for id, n, ctxs, k in (("empty", 0, 0, None), ("null_ctxs", 64, 0, EINVAL), ("ctxs_off_4", 64, CTXS + 1, EINVAL),
                           ("one_block", 256, CTXS, "md5_init_ctx"), ("two_blocks", 257, CTXS, "md5_init_ctx"),
                           ("grid_limit", 256 * MAXGRID, CTXS, "md5_init_ctx"),
                           ("grid_limit_plus_1", 256 * MAXGRID + 1, CTXS, EINVAL)):
        add("init_ctx." + id, "md5hip_init_ctx", [ctxs, n, STREAM],
            route_blocks_of_256("md5_init_ctx", n, ctxs and ctxs % 4 == 0, STREAM, ctxs, n), k)
    for id, n, ctxs, dig, k in (("empty", 0, 0, 0, None), ("null_ctxs", 64, 0, OUT, EINVAL),
                                ("null_digests", 64, CTXS, 0, EINVAL), ("ctxs_off_4", 64, CTXS + 2, OUT, EINVAL),
                                ("digests_off_16", 64, CTXS, OUT + 8, EINVAL),
                                ("one_block", 256, CTXS, OUT, "md5_final_ctx"),
                                ("two_blocks", 257, CTXS, OUT, "md5_final_ctx"),
                                ("grid_limit_plus_1", 256 * MAXGRID + 1, CTXS, OUT, EINVAL)):
        add("final_ctx." + id, "md5hip_final_ctx", [ctxs, n, dig, STREAM],
            route_blocks_of_256("md5_final_ctx", n, ctxs and dig and ctxs % 4 == 0 and dig % 16 == 0, STREAM,
                                ctxs, n, dig), k)

    # ---- the device-side order
    for id, n, lens, kmax, nxt, order, k in (
            ("empty", 0, 0, 0, 0, 0, None), ("null_lens", 100, 0, 64, NEXT, ORDER, EINVAL),
            ("null_next", 100, LENS, 64, 0, ORDER, EINVAL), ("null_order", 100, LENS, 64, NEXT, 0, EINVAL),
            ("kmax_at_limit", 1000, LENS, KMAX, NEXT, ORDER, "order_scatter"),
            ("kmax_past_limit", 1000, LENS, KMAX + 1, NEXT, ORDER, EINVAL),
            ("two_blocks", 257, LENS, 64, NEXT, ORDER, "order_scatter"),
            ("grid_limit_plus_1", 256 * MAXGRID + 1, LENS, 64, NEXT, ORDER, EINVAL)):
        add("order_device." + id, "md5hip_order_device", [lens, n, kmax, nxt, order, STREAM],
            route_blocks_of_256("order_scatter", n, lens and nxt and order and kmax <= KMAX, STREAM,
                                lens, n, kmax, nxt, order), k)
    # the stable order runs rocPRIM's host code past its checks: the argument errors only
    for id, n, lens, kmax, scratch, order, rc in (
            ("empty", 0, 0, 0, 0, 0, 0), ("null_lens", 100, 0, 64, SCRATCH, ORDER, EINVAL),
            ("null_scratch", 100, LENS, 64, 0, ORDER, EINVAL), ("null_order", 100, LENS, 64, SCRATCH, 0, EINVAL),
            ("kmax_0", 100, LENS, 0, SCRATCH, ORDER, EINVAL), ("kmax_past_limit", 100, LENS, KMAX + 1, SCRATCH, ORDER, EINVAL),
            ("n_past_int", 2**31, LENS, 64, SCRATCH, ORDER, EINVAL)):
        add("order_stable." + id, "md5hip_order_device_stable", [lens, n, kmax, scratch, 1 << 30, order, STREAM],
            (rc, [], None), EINVAL if rc else None)

    # ---- gather and fill: grid-stride past a cap
    for id, nseg in (("empty", 0), ("one", 1), ("at_cap", 65536), ("capped", 65537)):
        k = "gather_segments<4>" if nseg else None
        rec = [launch(k, min(nseg, 65536), 256, 0, STREAM, SEGS, nseg, OUT)] if nseg else []
        add("gather." + id, "md5hip_gather_launch", [SEGS, nseg, OUT, STREAM], (0, rec, k), k)
    for id, dst, nbytes, k in (("empty", 0, 0, None), ("null", 0, 64, EINVAL), ("nbytes_off_16", OUT, 24, EINVAL),
                               ("dst_off_16", OUT + 8, 64, EINVAL), ("one", OUT, 16, "fill_synthetic"),
                               ("two_blocks", OUT, 16 * 257, "fill_synthetic"),
                               ("under_cap", OUT, 16 * 256 * 8191, "fill_synthetic"),
                               ("at_cap", OUT, 16 * 256 * 8192, "fill_synthetic"),
                               ("capped", OUT, 16 * 256 * 8192 + 16, "fill_synthetic")):
        rec = [launch(k, min(ceil_div(nbytes // 16, 256), 8192), 256, 0, STREAM, dst, nbytes // 16, 0x5EED)] \
            if k == "fill_synthetic" else []
        add("fill." + id, "md5hip_fill_synthetic", [dst, nbytes, 0x5EED, STREAM],
            (EINVAL if k == EINVAL else 0, rec, None if k == EINVAL else k), k)

    # ---- page lists: run on the device by tests/test_page_kinds.py and the paged test files
    PAGED = "the paged kernels' results are checked by tests/test_page_kinds.py"
    COUNTS = (1, 32, 33, 64, 65, 64 * cus, 64 * cus + 1)
    KIND = {"md5": (DIGEST_MD5, PAGES_MD5), "crc32": (DIGEST_CRC32, PAGES_CRC), "md5crc32": (DIGEST_DUAL, PAGES_DUAL)}

    def digest_pages(id, kind, n, kernel, pages=PTRS, first=OFFS, lens=LENS, order=ORDER, P=16384, out_=OUT,
                     stream=STREAM):
        route = route_digest_pages(cus, kind, pages, first, lens, order, n, P, out_, stream)
        add("digest_pages." + id, "md5hip_digest_pages", [kind, pages, first, lens, order, n, P, out_, stream],
            route, kernel, why=PAGED)

    for name, (kind, k) in KIND.items():
        for n in COUNTS:
            digest_pages(f"{name}_n{n}", kind, n, k, P=(128, 384, 16384)[n % 3])
        digest_pages(f"{name}_no_order", kind, 100, k, order=0)
        digest_pages(f"{name}_empty", kind, 0, None, pages=0, first=0, lens=0, out_=0)
        digest_pages(f"{name}_null_pages", kind, 64, EINVAL, pages=0)
        digest_pages(f"{name}_null_first", kind, 64, EINVAL, first=0)
        digest_pages(f"{name}_null_lens", kind, 64, EINVAL, lens=0)
        digest_pages(f"{name}_null_out", kind, 64, EINVAL, out_=0)
        for P in (0, 64, PAGE_BYTES_MAX + 128):
            digest_pages(f"{name}_page_bytes_{P}", kind, 64, EINVAL, P=P)
        digest_pages(f"{name}_page_bytes_max", kind, 64, k, P=PAGE_BYTES_MAX)
        digest_pages(f"{name}_grid_limit", kind, 64 * MAXGRID, k)
        digest_pages(f"{name}_grid_limit_plus_1", kind, 64 * MAXGRID + 1, EINVAL)
        digest_pages(f"{name}_null_stream", kind, 65, k, stream=0)
    digest_pages("md5_out_off_16", DIGEST_MD5, 64, EINVAL, out_=OUT + 8)
    digest_pages("md5crc32_out_off_16", DIGEST_DUAL, 64, EINVAL, out_=OUT + 8)
    digest_pages("crc32_out_off_4", DIGEST_CRC32, 64, EINVAL, out_=OUT + 2)
    digest_pages("crc32_out_on_4", DIGEST_CRC32, 64, PAGES_CRC, out_=OUT + 4)
    digest_pages("kind_3", 3, 64, EINVAL)
    digest_pages("kind_minus_1", 2**32 - 1, 64, EINVAL)
    digest_pages("kind_3_empty", 3, 0, None)                # n == 0 comes first

    def crc_pages(id, n, F, kernel, pages=PTRS, first=OFFS, lens=LENS, order=ORDER, P=16384, out_=OUT):
        route = route_crc_pages(cus, pages, first, lens, order, n, P, F, out_, STREAM)
        add("crc_pages." + id, "crc32hip_pages", [pages, first, lens, order, n, P, F, out_, STREAM], route, kernel,
            why=PAGED)

    for n in COUNTS:
        crc_pages(f"whole_n{n}", n, 0, PAGES_CRC)                       # the order goes through
        crc_pages(f"window_64_n{n}", n, 64, PAGES_FAST, P=(128, 384, 16384)[n % 3])
    for n in (32 * cus, 32 * cus + 1):                                  # ceil(n / 32) groups against the CUs
        crc_pages(f"window_128_n{n}", n, 128, PAGES_FAST)
    crc_pages("whole_no_order", 100, 0, PAGES_CRC, order=0)
    crc_pages("window_no_order", 100, 128, PAGES_FAST, order=0)
    for F in (4, 132, 1000, 1 << 20):                                   # any multiple of 4: one kernel
        crc_pages(f"window_{F}", 100, F, PAGES_FAST)
    for F in (0, 64):
        crc_pages(f"empty_f{F}", 0, F, None, pages=0, first=0, lens=0, out_=0)
        crc_pages(f"null_pages_f{F}", 64, F, EINVAL, pages=0)
        crc_pages(f"null_first_f{F}", 64, F, EINVAL, first=0)
        crc_pages(f"null_lens_f{F}", 64, F, EINVAL, lens=0)
        crc_pages(f"null_out_f{F}", 64, F, EINVAL, out_=0)
        crc_pages(f"out_off_4_f{F}", 64, F, EINVAL, out_=OUT + 2)
        for P in (0, 64, PAGE_BYTES_MAX + 128):
            crc_pages(f"page_bytes_{P}_f{F}", 64, F, EINVAL, P=P)
    crc_pages("fastcrc_6", 64, 6, EINVAL)
    crc_pages("fastcrc_130", 64, 130, EINVAL)
    crc_pages("window_grid_limit", 32 * MAXGRID, 64, PAGES_FAST)
    crc_pages("window_grid_limit_plus_1", 32 * MAXGRID + 1, 64, EINVAL)
    crc_pages("whole_grid_limit_plus_1", 64 * MAXGRID + 1, 0, EINVAL)

    def update_ctx_pages(id, n, kernel, ctxs=CTXS, pages=PTRS, first=OFFS, lens=LENS, P=16384, stream=STREAM):
        route = route_update_ctx_pages(cus, ctxs, pages, first, lens, n, P, stream)
        add("update_ctx_pages." + id, "md5hip_update_ctx_pages", [ctxs, pages, first, lens, n, P, stream], route,
            kernel, why=PAGED)

    for n in COUNTS:
        update_ctx_pages(f"n{n}", n, PAGES_CTX, P=(128, 384, 16384)[n % 3])
    update_ctx_pages("empty", 0, None, ctxs=0, pages=0, first=0, lens=0)
    update_ctx_pages("null_ctxs", 64, EINVAL, ctxs=0)
    update_ctx_pages("null_pages", 64, EINVAL, pages=0)
    update_ctx_pages("null_first", 64, EINVAL, first=0)
    update_ctx_pages("null_lens", 64, EINVAL, lens=0)
    update_ctx_pages("ctxs_off_4", 64, EINVAL, ctxs=CTXS + 2)
    for P in (0, 64, PAGE_BYTES_MAX + 128):
        update_ctx_pages(f"page_bytes_{P}", 64, EINVAL, P=P)
    update_ctx_pages("page_bytes_max", 64, PAGES_CTX, P=PAGE_BYTES_MAX)
    update_ctx_pages("grid_limit", 64 * MAXGRID, PAGES_CTX)
    update_ctx_pages("grid_limit_plus_1", 64 * MAXGRID + 1, EINVAL)
    update_ctx_pages("null_stream", 65, PAGES_CTX, stream=0)
    return out


# ------------------------------------------------------------------ the kernels' own claims
# block: the one block size the kernel's indexing is written for
EXACT_BLOCK = {
    # xdma16_frame strides by gridDim.x * 12 and takes wave w's image at w * 8192: twelve waves
    "md5hip::crc32_fixed_xdma16": 768, "md5hip::crc32_desc_xdma16": 768, "md5hip::crc32_fast_xdma16": 768,
    "md5hip::md5crc32_fixed_xdma16": 768, "md5hip::md5crc32_desc_xdma16<true>": 768,
    "md5hip::md5crc32_desc_xdma16<false>": 768,
    # the bare s_barrier hand-over of a fed pair counts on exactly its two waves
    "md5hip::md5_desc_fed<true>": 128, "md5hip::md5_desc_fed<false>": 128, "md5hip::md5_update_ctx_fed": 128,
    "md5hip::md5crc32_fedsplit<true>": 128, "md5hip::md5crc32_fedsplit<false>": 128,
    # four 8 KiB images for four waves; BALANCED's one wave per SIMD
    "md5hip::md5_fixed_xdma1nt": 256, "md5hip::md5_desc_balanced_t<4, 2, 2>": 256,
    # md5_pages.hip: 'one wave per workgroup with its 8 KiB image'; 'XDMA16's frame ... twelve waves' images';
    # 'crc32_fast_pipe's frame: the perm tables alone in LDS, sixteen waves per CU'
    PAGES_MD5: 64, PAGES_CTX: 64, PAGES_CRC: 768, PAGES_DUAL: 768, PAGES_FAST: 1024,
}
LDS_PER_CU = 160 * 1024
# workgroups a CU holds by LDS: (kernel, count, the comment it restates)
WORKGROUPS_PER_CU = [
    ("md5hip::md5_desc_balanced_t<4, 2, 2>", 1,
     "BalancedCfg: 'the workgroup asks for more than half the CU's LDS, so a CU runs exactly one'"),
    ("md5hip::crc32_fixed_xdma16", 1, "XDMA16: 'One 768-thread workgroup per CU (160 KiB LDS)'"),
    ("md5hip::crc32_desc_xdma16", 1, "XDMA16: 'One 768-thread workgroup per CU (160 KiB LDS)'"),
    ("md5hip::crc32_fast_xdma16", 1, "XDMA16: 'One 768-thread workgroup per CU (160 KiB LDS)'"),
    ("md5hip::md5crc32_fixed_xdma16", 1, "md5crc32hip_fixed: 'XDMA16's 768-thread workgroup per CU'"),
    ("md5hip::md5crc32_desc_xdma16<true>", 1, "md5crc32hip_fixed: 'XDMA16's 768-thread workgroup per CU'"),
    ("md5hip::md5crc32_desc_xdma16<false>", 1, "md5crc32hip_fixed: 'XDMA16's 768-thread workgroup per CU'"),
    ("md5hip::crc32_split<true>", 2, "crc_split_grid: 'grid-stride past 8 [waves] per CU'"),
    ("md5hip::crc32_split<false>", 2, "crc_split_grid: 'grid-stride past 8 [waves] per CU'"),
    ("md5hip::crc32_fast_pipe", 2, "crc32_fast_pipe: the 16 table copies (64 KiB) of a 1,024-thread workgroup"),
    ("md5hip::md5crc32_fedsplit<true>", 2, "md5crc32_fedsplit: 'One 64 KiB LDS array ... so a CU holds two workgroups'"),
    ("md5hip::md5crc32_fedsplit<false>", 2, "md5crc32_fedsplit: 'One 64 KiB LDS array ... so a CU holds two workgroups'"),
    (PAGES_FAST, 2, "crc32_pages_fast: 'the perm tables alone in LDS, sixteen waves per CU' (64 KiB a workgroup)"),
    (PAGES_CRC, 1, "pages_xdma16: 'the 64 KiB tables beside twelve waves' images, one workgroup per CU'"),
    (PAGES_DUAL, 1, "pages_xdma16: 'the 64 KiB tables beside twelve waves' images, one workgroup per CU'"),
]
# waves per SIMD by registers: (kernel, 'eq' or 'ge', count, the comment it restates)
WAVES_PER_SIMD = [
    ("md5hip::md5_desc_xdma", "eq", 4,
     "md5_desc_xdma: 'claiming VGPRs up to v127 (an empty asm clobber) makes the register file cap it at 4 per SIMD'"),
    ("md5hip::md5_update_ctx", "eq", 4,
     "md5_update_ctx: 'its VGPRs (just under 128) hold it at 4 waves per SIMD'"),
    ("md5hip::md5_desc_lines", "eq", 3,
     "md5_desc_lines: 'The second line of registers costs occupancy (3 waves per SIMD instead of 4)'"),
    ("md5hip::md5_desc_hybrid", "eq", 3, "md5_desc_xdma: 'HYBRID's 163 VGPRs, 3 per SIMD'"),
    ("md5hip::md5_fixed_xdma1nt", "ge", 5, "md5_fixed_xdma1nt: amdgpu_waves_per_eu(5)"),
    ("md5hip::md5crc32_fedsplit<true>", "eq", 3,
     "md5crc32_fedsplit: '163 VGPRs ... and no AGPRs are three waves per SIMD'"),
    ("md5hip::md5crc32_fedsplit<false>", "eq", 3,
     "md5crc32_fedsplit: '163 VGPRs ... and no AGPRs are three waves per SIMD'"),
    (PAGES_MD5, "eq", 4, "md5_pages_xdma: 'held at 4 waves per SIMD by the register file, as md5_desc_xdma'"),
    (PAGES_CTX, "eq", 4, "md5_update_ctx_pages: 'held at 4 waves per SIMD by the register file'"),
    (PAGES_FAST, "ge", 4, "crc32_pages_fast: 'VGPRs: 128 at 16 waves per CU' (four per SIMD)"),
    (PAGES_CRC, "ge", 3, "pages_xdma16: XDMA16's frame, twelve waves per CU (three per SIMD)"),
    (PAGES_DUAL, "ge", 3, "pages_xdma16: XDMA16's frame, twelve waves per CU (three per SIMD)"),
]


def waves_per_simd(vgprs, agprs):
    """Waves a SIMD holds by registers on gfx950: 512 per lane, unified, in
    granules of 8."""
    alloc = ceil_div(vgprs + agprs, 8) * 8
    return min(8, 512 // alloc)
