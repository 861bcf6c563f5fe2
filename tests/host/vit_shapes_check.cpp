// Stand-alone host program over strique_amd/csrc/vit_model.h (no HIP): which kernel shape a model runs on, which decode modes a shape
// has, and that the shape table agrees with itself.  Built and run under ASan/UBSan by tests/test_vit_shapes_host.py; exits 0 when
// every check holds.  With --modes it prints one line "row mode" for every pair vit_mode_ok has (rows 0 .. VIT_LANE_SHAPES - 1, then the
// general and the register-resident shape) and nothing else: tests/test_vit_mode_cases_host.py holds its cases against that list.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "../../strique_amd/csrc/vit_model.h"

using namespace strq;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static VitModel dims(int e, int s, std::initializer_list<int> e_deg, std::initializer_list<int> s_deg)
{
    VitModel m; std::memset(&m, 0, sizeof(m));
    m.epl = e; m.spl = s; m.unit_state[0] = m.unit_state[1] = -1; m.rec_state = -1;
    int i = 0; for (int d : e_deg) m.e_deg[i++] = d;
    i = 0; for (int d : s_deg) m.s_deg[i++] = d;
    return m;
}

// the flanked-repeat model at the edge of the packed shapes: slots 2 and 3 flat
static VitModel flanked()
{
    VitModel m = dims(4, 2, {6, 5, 3, 3}, {2, 2});
    m.e_flat[2] = m.e_flat[3] = 1;
    return m;
}

static void shape_choice()
{
    VitModel m = flanked();
    CHECK(vit_shape_base(m) == 7);
    m = flanked(); m.e_flat[3] = 0; CHECK(vit_shape_base(m) == 5);
    m = flanked(); m.epl = 3; CHECK(vit_shape_base(m) == 5);
    m = flanked(); m.silent_counted = 1; CHECK(vit_shape_base(m) == 0);
    m = flanked(); m.s_deg[0] = 3; CHECK(vit_shape_base(m) == 0);
    m = flanked(); m.e_deg[1] = 6; CHECK(vit_shape_base(m) == 0);
    m = flanked(); m.e_deg[0] = 7; CHECK(vit_shape_base(m) == 3);
    CHECK(vit_shape_base(dims(1, 1, {5}, {1})) == 6);
    CHECK(vit_shape_base(dims(1, 1, {6}, {1})) == 1);
    CHECK(vit_shape_base(dims(1, 1, {5}, {2})) == 1);
    CHECK(vit_shape_base(dims(1, 2, {5}, {1, 1})) == 2);
    CHECK(vit_shape_base(dims(2, 2, {5, 5}, {5, 1})) == 3);
    CHECK(vit_shape_base(dims(5, 4, {5, 5, 5, 5, 5}, {1, 1, 1, 1})) == 4);
    CHECK(vit_shape_base(dims(4, 2, {9, 5, 3, 3}, {2, 2})) == -1);
    CHECK(vit_shape_base(dims(4, 2, {6, 5, 3, 3}, {9, 2})) == -1);
    CHECK(vit_shape_of(dims(4, 2, {9, 5, 3, 3}, {2, 2})) == -1);
    // csr wins whatever else is set; single_stage flags lane shapes only
    m = flanked(); m.csr = 1; m.single_stage = 1; CHECK(vit_shape_of(m) == 8 && VIT_SHAPE_CSR == 8 && VIT_SHAPE_G2 == 9);
    m = dims(4, 2, {9, 9, 9, 9}, {9, 9}); m.csr = 1; CHECK(vit_shape_of(m) == VIT_SHAPE_CSR);
    m = flanked(); CHECK(vit_shape_of(m) == 7);
    m.single_stage = 1; CHECK(vit_shape_of(m) == (7 | VIT_SHAPE_SS));
    CHECK(vit_shape_family(7 | VIT_SHAPE_SS) == VIT_FAMILY_LANE && vit_shape_family(VIT_SHAPE_CSR) == VIT_FAMILY_CSR);
    CHECK(vit_shape_family(VIT_SHAPE_G2) == VIT_FAMILY_G2 && vit_shape_family(-1) == VIT_FAMILY_NONE && vit_shape_family(10) == VIT_FAMILY_NONE);
}

static void mode_table()
{
    CHECK(VIT_COUNT == 0 && VIT_BACKPTR == 1 && VIT_MARK == 2 && VIT_HUB == 3 && VIT_UNIT == 4);
    for (int ss = 0; ss <= VIT_SHAPE_SS; ss += VIT_SHAPE_SS) {
        for (int id = -1; id <= 12; ++id) {
            for (int mode = -1; mode <= 6; ++mode) {
                bool want = false;
                const bool lane = id >= 0 && id <= 7;
                if (mode == VIT_COUNT || mode == VIT_MARK) want = lane || id == 8 || id == 9;
                else if (mode == VIT_BACKPTR) want = lane || id == 8;
                else if (mode == VIT_HUB) want = id == 1 || id == 2 || id == 6;
                else if (mode == VIT_UNIT) want = id == 0 || id == 2 || id == 3 || id == 4 || id == 5 || id == 7 || id == 9;
                const int shape = id < 0 ? id : (id | ss);
                CHECK(vit_mode_ok(shape, mode) == want);
            }
        }
    }
}

static void shape_for()
{
    VitG2 image; std::memset(&image, 0, sizeof(image));
    for (int g2_mark = 0; g2_mark <= 1; ++g2_mark) {
        for (int g2_unit = 0; g2_unit <= 1; ++g2_unit) {
            VitModel m = flanked(); m.g2 = &image; m.g2_mark = g2_mark; m.g2_unit = g2_unit;
            CHECK(vit_shape_for(m, VIT_COUNT, true) == VIT_SHAPE_G2);
            CHECK(vit_shape_for(m, VIT_MARK, true) == (g2_mark ? (int)VIT_SHAPE_G2 : 7));
            CHECK(vit_shape_for(m, VIT_UNIT, true) == (g2_unit ? (int)VIT_SHAPE_G2 : 7));
            CHECK(vit_shape_for(m, VIT_BACKPTR, true) == 7 && vit_shape_for(m, VIT_HUB, true) == 7);
            for (int mode = VIT_COUNT; mode <= VIT_UNIT; ++mode) CHECK(vit_shape_for(m, (VitMode)mode, false) == 7);
            m.g2 = nullptr;          // no image: the flags alone do nothing
            for (int mode = VIT_COUNT; mode <= VIT_UNIT; ++mode) CHECK(vit_shape_for(m, (VitMode)mode, true) == 7);
        }
    }
    // unit decodes: the model-level conditions and the shape's
    VitModel m = flanked(); m.unit_state[0] = 3; m.unit_state[1] = 9;
    CHECK(vit_unit_ok(m, 7) && vit_unit_ok(m, 0 | VIT_SHAPE_SS) && !vit_unit_ok(m, 1) && !vit_unit_ok(m, 6) && !vit_unit_ok(m, VIT_SHAPE_CSR) && !vit_unit_ok(m, -1));
    CHECK(!vit_unit_ok(m, VIT_SHAPE_G2));          // no image
    m.g2 = &image; CHECK(!vit_unit_ok(m, VIT_SHAPE_G2));
    m.g2_unit = 1; CHECK(vit_unit_ok(m, VIT_SHAPE_G2));
    m.silent_counted = 1; CHECK(!vit_unit_ok(m, VIT_SHAPE_G2) && !vit_unit_ok(m, 0));
    m.silent_counted = 0; m.unit_state[1] = -1; CHECK(!vit_unit_ok(m, 7));
    // the route of the modification pass: a model of at most two emitting slots that lands on a wider shape has no hub decode there
    // (it takes the back-pointer route)
    CHECK(vit_shape_base(dims(2, 3, {5, 5}, {1, 1, 1})) == 3 && !vit_mode_ok(3, VIT_HUB) && vit_mode_ok(3, VIT_BACKPTR));
}

// every model dimension the cascade can meet: the chosen row covers it
static void consistency()
{
    for (int id = 0; id < VIT_LANE_SHAPES; ++id) {
        CHECK(VIT_SHAPES[id].id == id);
        CHECK(vit_shape_silent_slots(id) == VIT_SHAPES[id].spl && vit_shape_silent_slots(id | VIT_SHAPE_SS) == VIT_SHAPES[id].spl);
        const VitFwdShape& f = VIT_FWD_SHAPES[VIT_SHAPES[id].fwd];          // the forward instance covers the row
        CHECK(f.epl >= VIT_SHAPES[id].epl && f.spl >= VIT_SHAPES[id].spl && f.ds >= VIT_SHAPES[id].ds);
        for (int i = 0; i < VIT_SHAPES[id].epl; ++i) CHECK(f.de >= vit_slot_deg(VIT_SHAPES[id], i));
        bool tried = false;
        for (int t : VIT_SHAPE_TRY) tried = tried || t == id;
        CHECK(tried);
    }
    CHECK(vit_shape_silent_slots(VIT_SHAPE_CSR) == 0 && vit_shape_silent_slots(VIT_SHAPE_G2) == 0 && vit_shape_silent_slots(-1) == 0);
    long n = 0, fitted = 0;
    for (int e = 1; e <= 8; ++e) for (int s = 1; s <= 4; ++s)
    for (int d0 = 0; d0 <= 9; ++d0) for (int d1 = 0; d1 <= 9; ++d1) for (int dlo = 0; dlo <= 9; ++dlo) for (int ds = 0; ds <= 9; ++ds)
    for (int flags = 0; flags < 4; ++flags) {
        // slot groups: slot 0, the rest of the first half, the second half
        VitModel m; std::memset(&m, 0, sizeof(m));
        m.epl = e; m.spl = s; m.silent_counted = flags & 1;
        for (int i = 0; i < e; ++i) { m.e_deg[i] = i == 0 ? d0 : (i < (e + 1) / 2 ? d1 : dlo); m.e_flat[i] = (flags & 2) && i >= (e + 1) / 2; }
        for (int i = 0; i < s; ++i) m.s_deg[i] = i == 0 ? ds : ds / 2;
        const int b = vit_shape_base(m);
        ++n;
        if (b < 0) {          // only what no row holds is refused
            bool over = false;
            for (int i = 0; i < e; ++i) over = over || m.e_deg[i] > 8;
            for (int i = 0; i < s; ++i) over = over || m.s_deg[i] > 8;
            CHECK(over);
            continue;
        }
        ++fitted;
        CHECK(b < VIT_LANE_SHAPES);
        const VitShape& r = VIT_SHAPES[b];
        CHECK(r.epl >= e && r.spl >= s && r.ds >= ds);
        for (int i = 0; i < e; ++i) CHECK(vit_slot_deg(r, i) >= m.e_deg[i]);
        CHECK(vit_silent_counted(r.de_hi) || !m.silent_counted);
        if (vit_lo_flat(r.de_lo)) for (int i = (r.epl + 1) / 2; i < r.epl; ++i) CHECK(i < e && m.e_flat[i]);
    }
    CHECK(n > 100000 && fitted > n / 2);
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--modes") == 0) {
        for (int id = 0; id <= VIT_SHAPE_G2; ++id)
            for (int mode = VIT_COUNT; mode <= VIT_UNIT; ++mode) if (vit_mode_ok(id, mode)) std::printf("%d %d\n", id, mode);
        return 0;
    }
    shape_choice();
    mode_table();
    shape_for();
    consistency();
    if (failures) { std::fprintf(stderr, "%d checks failed\n", failures); return 1; }
    std::printf("vit_shapes ok\n");
    return 0;
}
