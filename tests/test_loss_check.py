"""CPU checks of tests/loss_check.py, the comparison behind tests/test_losses_gpu.py:
  * the conditions on the measured constants (r32 <= 16) and on the sentinels (>= 100 x tolerance), for every case of the tables;
  * the float64 reference rounded to float32 passes;
  * eight faulted results, (a) to (h), each the rounded reference with ONE fault of the kind the kernels' reduction shapes invite:
    the comparison must refuse each and name the tensor.  For (a) and (h) the rule the loss tests used before (1e-4 of the
    tensor's maximum) is shown to accept the same faulted tensor.
"""
import pytest
import torch

import loss_check as L

ALL_CASES = [c.name for c in L.INFONCE_CASES + L.CE_CASES + L.ORI_CASES]


def rounded(ref):
    """what a perfect float32 implementation would return"""
    out = dict(loss=ref.loss.float(), grad=ref.grad.float())
    if ref.kind == "infonce":
        out["rows"] = ref.rows().float()
    return out


def refused(ref, tensor, **got):
    """check() must refuse `got` and name `<case> <tensor>`; returns the message"""
    with pytest.raises(AssertionError) as e:
        L.check(ref, **got)
    assert "%s %s" % (ref.name, tensor) in str(e.value), str(e.value)
    return str(e.value)


def nce_rows(ref, z, den, a):
    """[4B + 4] float32 statistics the finish kernel would write from (faulted) merged partials"""
    r = ref.rows()
    b = ref.case.b
    r[0:4 * b:4], r[1:4 * b:4], r[2:4 * b:4], r[4 * b] = a - torch.log(z) * den, den, z, den.sum()
    return r.float()


def nce_a(ref):
    return (ref.tt * ref.labm).sum(1)


# ----------------------------------------------------------------------------------------------------------------------
# conditions
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_constants_sentinels_and_the_rounded_reference(name):
    ref = L.cached_ref(name)
    print("%s: r32 gradient %.2f, values %.2f -> c = %.1f, c_v = %.1f" % (name, ref.r32_grad, ref.r32_val, ref.c, ref.c_v))
    assert ref.r32_grad <= L.R32_CAP and ref.r32_val <= L.R32_CAP, "the float32 oracle is %.1f / %.1f x u model away from float64" % (
        ref.r32_grad, ref.r32_val)
    assert ref.c == 4 * max(ref.r32_grad, 2.0) and ref.c_v == 4 * max(ref.r32_val, 4.0)
    margins = L.sentinel_margins(ref)
    print("%s: leaving out one sentinel moves %s x the tolerance" % (name, {k: "%.0f" % v for k, v in margins.items()}))
    assert set(margins) == ({"z_b", "num_b"} if ref.kind == "infonce" else {"term_b"})
    assert min(margins.values()) >= L.SENTINEL_MARGIN, margins
    ratios = L.check(ref, **rounded(ref))
    assert max(ratios.values()) <= 1.0 / min(ref.c, ref.c_v) + 1e-9          # one rounding: half an ulp <= u |ref| <= u model


def test_case_tables_hold_what_the_kernels_branch_on():
    by = {c.name: c for c in L.INFONCE_CASES}
    assert by["nce_b3_n5119"].n % 4 == 3 and by["nce_b3_n5119"].n < L.NCE_CH
    c = by["nce_b6_n16388"]
    assert c.n == 2 * L.NCE_CH + 4 and c.b > 4 and c.g == 1e4 / 6
    s, lab = L.infonce_inputs(c)
    assert float(lab[c.edge]) == float(torch.tensor(0.01, dtype=torch.float32)) and float(s[c.edge]) == 1.0
    assert not bool((lab[4] > 1e-2).any()) and bool((lab[5] > 1e-2).any())
    assert by["nce_b70_n1280"].b > 64 and by["nce_b70_n1280"].t == 0.07
    assert -(-by["nce_b2_66chunks"].n // L.NCE_CH) == 66 and -(-by["nce_b2_level6"].n // L.NCE_CH) == 160
    pos = L.sentinel_positions(16388, L.NCE_CH)
    assert pos == [0, 8191, 8192, 16383, 16384, 16385, 16386, 16387]
    assert L.sentinel_positions(5119) == [0, 5116, 5117, 5118]
    assert [c.n % 1024 for c in L.CE_CASES] == [0, 3, 0] and [c.b for c in L.CE_CASES] == [5, 2, 66]
    assert [(c.b, c.h * c.w) for c in L.ORI_CASES] == [(5, 512 * 512), (3, 1001), (66, 1024)]


# ----------------------------------------------------------------------------------------------------------------------
# faults
# ----------------------------------------------------------------------------------------------------------------------
def test_fault_a_vector_tail_left_out():
    """(a) the last n % 4 elements left out of z, their gradients left unwritten (zeros)"""
    ref = L.cached_ref("nce_b3_n5119")
    k = ref.case.n % 4
    z = ref.z - torch.exp(ref.tt[:, -k:]).sum(1)
    refused(ref, "rows.", rows=nce_rows(ref, z, ref.den, nce_a(ref)))
    grad = L.infonce_grad_formula(ref, z=z)
    grad[:, -k:] = 0
    refused(ref, "grad", grad=grad.float())
    # a tail nobody would miss (scores -3, labels 0): the statistics do not move, the unwritten gradients are ~1e-13 of the
    # largest.  The old rule accepts the tensor, the elementwise one does not.
    quiet = L.InfoNCERef(ref.case, *L.infonce_inputs(ref.case, quiet_tail=True))
    grad = quiet.grad.float()
    assert float(grad[:, -k:].abs().min()) > 0
    grad[:, -k:] = 0
    assert L.old_rule_passes(grad, quiet.grad, 1e-4)
    refused(quiet, "grad", grad=grad)
    L.check(quiet, **rounded(quiet))


def test_fault_b_chunk_beyond_lane_63_left_out_of_the_merge():
    """(b) chunk 65 (the 8-element last chunk) left out of row 1's merge"""
    ref = L.cached_ref("nce_b2_66chunks")
    lo = 65 * L.NCE_CH
    z, den, a = ref.z.clone(), ref.den.clone(), nce_a(ref)
    z[1] -= torch.exp(ref.tt[1, lo:]).sum()
    den[1] -= ref.labm[1, lo:].sum()
    a[1] -= (ref.tt[1, lo:] * ref.labm[1, lo:]).sum()
    rows = nce_rows(ref, z, den, a)
    refused(ref, "rows.", rows=rows)
    refused(ref, "loss", loss=(-(rows[0:8:4].double().sum()) / den.sum()).float())
    refused(ref, "grad", grad=L.infonce_grad_formula(ref, z=z, den=den, d=den.sum()).float())


def test_fault_c_rows_beyond_64_left_out_of_d():
    """(c) rows b >= 64 left out of the batch sums"""
    ref = L.cached_ref("nce_b70_n1280")
    d = ref.den[:64].sum()
    rows = ref.rows()
    rows[4 * 70] = d
    refused(ref, "rows.D", rows=rows.float())
    refused(ref, "loss", loss=(-ref.num[:64].sum() / d).float())
    refused(ref, "grad", grad=L.infonce_grad_formula(ref, d=d).float())


def test_fault_d_second_pass_of_the_row_loop_reuses_z():
    """(d) rows b >= 4 take row b - 4's z"""
    ref = L.cached_ref("nce_b6_n16388")
    z = ref.z.clone()
    z[4:] = ref.z[:2]
    refused(ref, "rows.", rows=nce_rows(ref, z, ref.den, nce_a(ref)))
    msg = refused(ref, "grad", grad=L.infonce_grad_formula(ref, z=z).float())
    assert "worst at (5," in msg                       # row 4 has no positives: its gradient is zero whatever z is


def test_fault_e_cross_entropy_backward_assumes_normalised_labels():
    """(e) ls = 1 with labels whose rows sum to 0.3 .. 3"""
    ref = L.cached_ref("ce_b66_n4096")
    grad = ref.g / ref.case.b * (ref.p - ref.lab.double())
    refused(ref, "grad", grad=grad.float())


def test_fault_f_gradient_divided_by_the_wrong_batch():
    """(f) 64 instead of 66"""
    for name in ("ori_b66_hw1024", "ce_b66_n4096"):
        ref = L.cached_ref(name)
        refused(ref, "grad", grad=(ref.grad * 66 / 64).float())


def test_fault_g_label_equal_to_the_threshold_counted():
    """(g) `>=` instead of `>` at the label equal to 0.01f"""
    ref = L.cached_ref("nce_b6_n16388")
    b, j = ref.case.edge
    assert float(ref.labm[b, j]) == 0.0
    labm = ref.labm.clone()
    labm[b, j] = ref.lab[b, j].double()
    den = labm.sum(1)
    refused(ref, "rows.", rows=nce_rows(ref, ref.z, den, (ref.tt * labm).sum(1)))
    msg = refused(ref, "grad", grad=L.infonce_grad_formula(ref, den=den, d=den.sum(), labm=labm).float())
    print(msg)


def test_fault_h_one_softmax_tail_element_off_by_one_percent():
    """(h) one element without a label, far down the row's softmax, 1 % off"""
    ref = L.cached_ref("nce_b3_n5119")
    cand = torch.where(ref.labm[0] == 0, ref.tt[0], torch.full_like(ref.tt[0], float("inf")))
    j = int(cand.argmin())
    assert float(ref.grad[0, j]) > 0 and float(ref.grad[0, j]) < 1e-4 * float(ref.grad.abs().max())
    grad = ref.grad.clone()
    grad[0, j] *= 1.01
    grad = grad.float()
    assert L.old_rule_passes(grad, ref.grad, 1e-4)
    msg = refused(ref, "grad", grad=grad)
    assert "worst at (0, %d)" % j in msg
    # the same for a cross-entropy row: an element whose softmax term outweighs its label
    ref = L.cached_ref("ce_b2_n4099")
    share = ref.ls[:, None] * ref.p / (ref.lab.double() + 1e-300)
    share[:, L.sentinel_positions(ref.case.n)] = 0
    j = int(share[1].argmax())
    grad = ref.g / ref.case.b * (ref.ls[:, None] * ref.p - ref.lab.double())
    grad[1, j] = ref.g / ref.case.b * (ref.ls[1] * ref.p[1, j] * 1.01 - ref.lab[1, j].double())
    assert L.old_rule_passes(grad.float(), ref.grad, 1e-4)
    assert "worst at (1, %d)" % j in refused(ref, "grad", grad=grad.float())
