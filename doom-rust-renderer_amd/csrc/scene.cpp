// scene.cpp — IWAD container, map lumps and graphics decode into dg::Scene.
//
// On-disk formats: SURVEY.md Appendix B (reference loaders: src/wad.rs, src/map/*.rs, src/graphics/*.rs).
// Where the reference's HashMap/Vec semantics decide a result (duplicate lump or texture names, first map
// marker, lazy texture composition with later patches overwriting — including with transparent texels) the
// same choice is made here; where the reference would panic the loader throws and the C-ABI returns DG_ERR_WAD.
#include "scene.hpp"

#include <algorithm>
#include <array>
#include <cctype>
#include <cmath>
#include <cstring>
#include <map>
#include <stdexcept>
#include <unordered_map>

namespace dg {
namespace {

struct LoadError : std::runtime_error { using std::runtime_error::runtime_error; };

std::string upper(const std::string &s) {
    std::string r = s;
    for (auto &c : r) c = (char)std::toupper((unsigned char)c);
    return r;
}

struct Lump { std::string name; uint32_t off, size; };

struct Wad {
    const std::vector<uint8_t> &b;
    std::vector<Lump> dir;
    std::unordered_map<std::string, int> by_name;  // last lump of a name wins (HashMap insert, src/wad.rs:153-154)

    explicit Wad(const std::vector<uint8_t> &bytes) : b(bytes) {
        if (b.size() < 12) throw LoadError("file shorter than a WAD header");
        if (std::memcmp(b.data(), "IWAD", 4) != 0) throw LoadError("Unhandled WAD file type (src/wad.rs:90-92)");
        uint32_t n = u32(4), doff = u32(8);
        need(doff, (size_t)n * 16, "directory");
        dir.reserve(n);
        for (uint32_t i = 0; i < n; i++) {
            size_t e = (size_t)doff + (size_t)i * 16;
            Lump l{upper(name8(e + 8)), u32(e), u32(e + 4)};
            by_name[l.name] = (int)i;
            dir.push_back(std::move(l));
        }
    }
    void need(size_t off, size_t n, const char *what) const {
        if (off > b.size() || n > b.size() - off) throw LoadError(std::string("out-of-file read in ") + what);
    }
    uint8_t u8(size_t o) const { need(o, 1, "byte"); return b[o]; }
    int16_t i16(size_t o) const { need(o, 2, "i16"); return (int16_t)(uint16_t)(b[o] | (b[o + 1] << 8)); }
    uint32_t u32(size_t o) const {
        need(o, 4, "u32");
        return (uint32_t)b[o] | ((uint32_t)b[o + 1] << 8) | ((uint32_t)b[o + 2] << 16) | ((uint32_t)b[o + 3] << 24);
    }
    // 8 bytes, NUL-terminated when shorter; case preserved (src/wad.rs:112-126)
    std::string name8(size_t o) const {
        need(o, 8, "name");
        size_t n = 0;
        while (n < 8 && b[o + n] != 0) n++;
        if (b[o + 7] != 0) n = 8;
        return std::string((const char *)&b[o], n);
    }
    int find(const std::string &name) const {
        auto it = by_name.find(upper(name));
        return it == by_name.end() ? -1 : it->second;
    }
    const Lump &map_lump(const std::string &map, int k) const {  // first marker + k (src/wad.rs:175-183)
        std::string m = upper(map);
        for (size_t i = 0; i < dir.size(); i++)
            if (dir[i].name == m) {
                if (i + (size_t)k >= dir.size()) break;
                const Lump &l = dir[i + (size_t)k];
                need(l.off, l.size, "map lump");
                return l;
            }
        throw LoadError("Could not find map lumps for " + map);
    }
};

struct Patch { int16_t ox, oy, pnum; };
struct TexDef { std::string name; int16_t w, h; std::vector<Patch> patches; };

// Row-major Option<u8> image while decoding; -1 = None.
struct Image {
    int w = 0, h = 0;
    std::vector<int16_t> px;
    Image(int w_, int h_) : w(w_), h(h_), px((size_t)std::max(w_, 0) * (size_t)std::max(h_, 0), (int16_t)-1) {}
    int16_t &at(int x, int y) { return px[(size_t)y * (size_t)w + (size_t)x]; }
    int16_t at(int x, int y) const { return px[(size_t)y * (size_t)w + (size_t)x]; }
};

struct Builder {
    Scene &sc;
    Wad wad;
    std::vector<std::string> pnames;
    std::vector<TexDef> texdefs;
    std::unordered_map<std::string, int> bitmap_by_key;
    std::unordered_map<std::string, int> flat_by_name;
    int first_sprite = -1, last_sprite = -1;

    explicit Builder(Scene &s) : sc(s), wad(s.wad) {}
    // A builder for a scene that is already loaded: the caches it needs, from what is in the scene
    static Builder resume(Scene &s) {
        Builder b(s);
        for (size_t i = 0; i < s.bitmap_names.size(); i++) b.bitmap_by_key[s.bitmap_names[i]] = (int)i;
        for (size_t i = 0; i < s.flat_names.size(); i++) b.flat_by_name[s.flat_names[i]] = (int)i;
        b.first_sprite = b.wad.find("S_START");
        b.last_sprite = b.wad.find("S_END");
        return b;
    }

    int add_bitmap(const std::string &key, const Image &im, int16_t left, int16_t top) {
        BitmapInfo bi;
        bi.w = im.w; bi.h = im.h; bi.left_offset = left; bi.top_offset = top;
        bi.texel_off = (uint32_t)sc.texel_idx.size();
        size_t n = (size_t)im.w * (size_t)im.h;
        sc.texel_idx.resize(sc.texel_idx.size() + n);
        sc.texel_opq.resize(sc.texel_opq.size() + n);
        for (int x = 0; x < im.w; x++)
            for (int y = 0; y < im.h; y++) {
                int16_t v = im.at(x, y);
                size_t o = bi.texel_off + (size_t)x * (size_t)im.h + (size_t)y;
                sc.texel_idx[o] = v < 0 ? 0 : (uint8_t)v;
                sc.texel_opq[o] = v < 0 ? 0 : 1;
                if (v < 0) bi.has_holes = 1;
            }
        sc.bitmaps.push_back(bi);
        sc.bitmap_names.push_back(key);
        int id = (int)sc.bitmaps.size() - 1;
        bitmap_by_key[key] = id;
        return id;
    }

    // Picture::new + read_pixels (src/graphics/pictures.rs:66-126)
    Image decode_picture(const std::string &lump_name, int16_t &left, int16_t &top) {
        int li = wad.find(lump_name);
        if (li < 0) throw LoadError("Could not find lump " + lump_name);
        size_t off = wad.dir[(size_t)li].off;
        int16_t w = wad.i16(off), h = wad.i16(off + 2);
        left = wad.i16(off + 4);
        top = wad.i16(off + 6);
        if (w < 0 || h < 0) throw LoadError("picture " + lump_name + " has a negative size");
        Image im(w, h);
        for (int col = 0; col < w; col++) {
            size_t co = off + wad.u32(off + 8 + (size_t)col * 4);
            for (;;) {
                uint8_t ytop = wad.u8(co);
                if (ytop == 0xff) break;
                uint8_t len = wad.u8(co + 1);
                for (int r = 0; r < len; r++) {
                    int y = r + ytop;
                    if (y >= h) throw LoadError("picture " + lump_name + ": post beyond height (reference index panic)");
                    im.at(col, y) = wad.u8(co + 3 + (size_t)r);
                }
                co += (size_t)len + 4;
            }
        }
        return im;
    }
    int picture_bitmap(const std::string &lump_name, bool mirrored) {
        std::string key = "P:" + upper(lump_name) + (mirrored ? ":M" : "");
        auto it = bitmap_by_key.find(key);
        if (it != bitmap_by_key.end()) return it->second;
        int16_t left, top;
        Image im = decode_picture(lump_name, left, top);
        if (mirrored) {  // Picture::mirror pictures.rs:129-147
            Image m(im.w, im.h);
            for (int y = 0; y < im.h; y++)
                for (int x = 0; x < im.w; x++) m.at(x, y) = im.at(im.w - 1 - x, y);
            im = std::move(m);
        }
        return add_bitmap(key, im, left, top);
    }

    // Textures::new: PNAMES + TEXTURE1 [+ TEXTURE2] (src/graphics/textures.rs:132-151,182-255)
    void load_texture_defs() {
        int pi = wad.find("PNAMES");
        if (pi < 0) throw LoadError("Could not find lump PNAMES");
        size_t po = wad.dir[(size_t)pi].off;
        uint32_t np = wad.u32(po);
        for (uint32_t i = 0; i < np; i++) pnames.push_back(wad.name8(po + 4 + (size_t)i * 8));
        for (const char *ln : {"TEXTURE1", "TEXTURE2"}) {
            int ti = wad.find(ln);
            if (ti < 0) {
                if (std::strcmp(ln, "TEXTURE1") == 0) throw LoadError("Could not find lump TEXTURE1");
                continue;
            }
            size_t base = wad.dir[(size_t)ti].off;
            uint32_t n = wad.u32(base);
            for (uint32_t i = 0; i < n; i++) {
                size_t o = base + wad.u32(base + 4 + 4 * (size_t)i);
                TexDef d;
                d.name = upper(wad.name8(o));
                d.w = wad.i16(o + 12);
                d.h = wad.i16(o + 14);
                int16_t pc = wad.i16(o + 20);
                for (int j = 0; j < pc; j++) {
                    size_t q = o + 22 + (size_t)j * 10;
                    d.patches.push_back(Patch{wad.i16(q), wad.i16(q + 2), wad.i16(q + 4)});
                }
                texdefs.push_back(std::move(d));
            }
        }
    }
    // Textures::get + Texture::load (textures.rs:154-179, 74-103).  Returns TEX_NONE for "-" is the caller's job.
    int texture_bitmap(const std::string &name) {
        std::string up = upper(name);
        std::string key = "T:" + up;
        auto it = bitmap_by_key.find(key);
        if (it != bitmap_by_key.end()) return it->second;
        const TexDef *d = nullptr;
        for (auto r = texdefs.rbegin(); r != texdefs.rend(); ++r)   // later definition replaced the earlier one
            if (r->name == up) { d = &*r; break; }
        if (!d) return TEX_UNKNOWN;
        if (d->w <= 0 || d->h <= 0) throw LoadError("texture " + up + " has a non-positive size");
        Image im(d->w, d->h);
        for (const Patch &p : d->patches) {
            if (p.pnum < 0 || (size_t)p.pnum >= pnames.size()) throw LoadError("texture " + up + ": patch number out of range");
            int16_t l, t;
            Image pic = decode_picture(pnames[(size_t)p.pnum], l, t);
            for (int x = 0; x < pic.w; x++)
                for (int y = 0; y < pic.h; y++) {
                    int16_t tx = (int16_t)(uint16_t)((uint16_t)x + (uint16_t)p.ox);
                    int16_t ty = (int16_t)(uint16_t)((uint16_t)y + (uint16_t)p.oy);
                    if (tx >= 0 && tx < d->w && ty >= 0 && ty < d->h) im.at(tx, ty) = pic.at(x, y);  // None overwrites too
                }
        }
        return add_bitmap(key, im, 0, 0);
    }
    int sidedef_texture(const std::string &name) { return name == "-" ? TEX_NONE : texture_bitmap(name); }

    // Flats::get + Flat::new (flats.rs:92-100,116-136)
    int flat(const std::string &name) {
        auto it = flat_by_name.find(name);
        if (it != flat_by_name.end()) return it->second;
        int li = wad.find(name);
        int id = FLAT_MISSING;
        if (li >= 0) {
            const Lump &l = wad.dir[(size_t)li];
            wad.need(l.off, 4096, "flat");
            id = (int)sc.flat_names.size();
            sc.flat_names.push_back(name);
            sc.flat_sky.push_back(name.find("SKY") != std::string::npos ? 1 : 0);
            sc.flat_pool.insert(sc.flat_pool.end(), sc.wad.begin() + l.off, sc.wad.begin() + l.off + 4096);
        }
        flat_by_name[name] = id;
        return id;
    }
};

// Animated flat lists (src/graphics/flats.rs:30-75; from p_spec.c)
const char *const kAnim[9][5] = {
    {"NUKAGE1", "NUKAGE2", "NUKAGE3", nullptr, nullptr},   {"FWATER1", "FWATER2", "FWATER3", "FWATER4", nullptr},
    {"SWATER1", "SWATER2", "SWATER3", "SWATER4", nullptr}, {"LAVA1", "LAVA2", "LAVA3", "LAVA4", nullptr},
    {"BLOOD1", "BLOOD2", "BLOOD3", nullptr, nullptr},      {"RROCK05", "RROCK06", "RROCK07", "RROCK08", nullptr},
    {"SLIME01", "SLIME02", "SLIME03", "SLIME04", nullptr}, {"SLIME05", "SLIME06", "SLIME07", "SLIME08", nullptr},
    {"SLIME09", "SLIME10", "SLIME11", "SLIME12", nullptr},
};
int anim_list_of(const std::string &name) {
    for (int l = 0; l < 9; l++)
        for (int k = 0; kAnim[l][k]; k++)
            if (name == kAnim[l][k]) return l;
    return -1;
}

// Animated wall lists (Doom's p_spec.c animdefs, wall entries, expanded to the frame names the stock IWADs hold between the first and the
// last name; restated, not checked against an id WAD — DESIGN.md §8b).  A list animates only when every member is a known texture.
const char *const kWallAnim[13][5] = {
    {"BLODGR1", "BLODGR2", "BLODGR3", "BLODGR4", nullptr},   {"SLADRIP1", "SLADRIP2", "SLADRIP3", nullptr, nullptr},
    {"BLODRIP1", "BLODRIP2", "BLODRIP3", "BLODRIP4", nullptr}, {"FIREWALA", "FIREWALB", "FIREWALL", nullptr, nullptr},
    {"GSTFONT1", "GSTFONT2", "GSTFONT3", nullptr, nullptr},  {"FIRELAV3", "FIRELAVA", nullptr, nullptr, nullptr},
    {"FIREMAG1", "FIREMAG2", "FIREMAG3", nullptr, nullptr},  {"FIREBLU1", "FIREBLU2", nullptr, nullptr, nullptr},
    {"ROCKRED1", "ROCKRED2", "ROCKRED3", nullptr, nullptr},  {"BFALL1", "BFALL2", "BFALL3", "BFALL4", nullptr},
    {"SFALL1", "SFALL2", "SFALL3", "SFALL4", nullptr},       {"WFALL1", "WFALL2", "WFALL3", "WFALL4", nullptr},
    {"DBRAIN1", "DBRAIN2", "DBRAIN3", "DBRAIN4", nullptr},
};
constexpr int kWallScrollSpecial = 48;   // "scroll texture left" (p_spec.c P_UpdateSpecials)

struct SpawnRow { int16_t id; const char *sprite; uint8_t frame, full_bright, is_null; };
const SpawnRow kSpawn[] = {
#include "../../data/mobj_spawn_table.inc"
};

// get_sky_texture (src/game.rs:199-227): regex `e(\d+)m(\d+)` searched anywhere, else `(\d\d)`, else SKY1.
const char *sky_name_for_map(const std::string &m) {
    for (size_t i = 0; i < m.size(); i++) {
        if (m[i] != 'e') continue;
        size_t j = i + 1, e = j;
        while (e < m.size() && std::isdigit((unsigned char)m[e])) e++;
        for (size_t k = e; k > j; k--)   // backtrack the greedy \d+ until 'm' + digit follows
            if (k + 1 < m.size() && m[k] == 'm' && std::isdigit((unsigned char)m[k + 1])) {
                long ep = std::strtol(m.substr(j, k - j).c_str(), nullptr, 10);
                return ep == 2 ? "SKY2" : ep == 3 ? "SKY3" : "SKY1";
            }
    }
    for (size_t i = 0; i + 1 < m.size(); i++)
        if (std::isdigit((unsigned char)m[i]) && std::isdigit((unsigned char)m[i + 1])) {
            int n = (m[i] - '0') * 10 + (m[i + 1] - '0');
            return n < 12 ? "SKY1" : n < 21 ? "SKY2" : "SKY3";
        }
    return "SKY1";
}

const float kPi = 3.14159265358979323846f;

}  // namespace

// Vertex::is_left_of_line for a node's partition (src/map/vertexes.rs:27-34, src/renderer/bsp.rs:15-19)
static inline bool left_of_partition(const NodeRec &n, float px, float py) {
    float v2x = n.x + n.dx, v2y = n.y + n.dy;
    float ax = px - n.x, ay = py - n.y;
    float bx = v2x - n.x, by = v2y - n.y;
    return ax * by - ay * bx <= 0.0f;
}

int Scene::sector_from_vertex(float x, float y) const {
    int ni = (int)nodes.size() - 1;
    for (;;) {
        const NodeRec &n = nodes[(size_t)ni];
        int16_t child = left_of_partition(n, x, y) ? n.lchild : n.rchild;
        if (child & (int16_t)0x8000) {
            const SubSectorRec &ss = subsectors[(size_t)(child & 0x7fff)];
            for (int k = 0; k < ss.count; k++) {
                const SegRec &sg = segs[(size_t)(ss.first + k)];
                const LinedefRec &ld = linedefs[(size_t)sg.linedef];
                int sd = sg.direction ? ld.back : ld.front;
                if (sd >= 0) return sidedefs[(size_t)sd].sector;
            }
            return -1;
        }
        ni = child & 0x7fff;
    }
}

// The flat tables of walk_core.h from the scene's records, by the rule of Scene::sector_from_vertex: the first seg of a leaf that has
// a sidedef on its side decides.
void Scene::build_walk_tables() {
    walk_nodes.resize(nodes.size());
    for (size_t i = 0; i < nodes.size(); i++) {
        const NodeRec &n = nodes[i];
        auto child = [](int16_t c) { return (c & (int16_t)0x8000) ? ~(int32_t)(c & 0x7fff) : (int32_t)(c & 0x7fff); };
        walk_nodes[i] = WalkNode{n.x, n.y, n.dx, n.dy, {child(n.rchild), child(n.lchild)}};
    }
    walk_leaves.assign(subsectors.size(), WalkLeaf{0.0f, 1u});
    walk_leaf_sector.assign(subsectors.size(), -1);
    for (size_t l = 0; l < subsectors.size(); l++) {
        const SubSectorRec &ss = subsectors[l];
        for (int k = 0; k < ss.count; k++) {
            const SegRec &sg = segs[(size_t)(ss.first + k)];
            const LinedefRec &ld = linedefs[(size_t)sg.linedef];
            const int sd = sg.direction ? ld.back : ld.front;
            if (sd < 0) continue;
            walk_leaves[l] = WalkLeaf{(float)sectors[(size_t)sidedefs[(size_t)sd].sector].floor_h, 0u};
            walk_leaf_sector[l] = sidedefs[(size_t)sd].sector;
            break;
        }
    }
}

int Scene::texture_id(const std::string &name) const {
    std::string key = "T:" + upper(name);
    for (size_t i = 0; i < bitmap_names.size(); i++)
        if (bitmap_names[i] == key) return (int)i;
    return TEX_UNKNOWN;
}
int Scene::flat_id(const std::string &name, float timestamp) const {
    int l = anim_list_of(name);
    std::string want = name;
    if (l >= 0) {
        size_t n = 0;
        while (kAnim[l][n]) n++;
        float t = timestamp * 3.0f;
        size_t cyc = !(t > 0.0f) ? 0 : (t >= 18446744073709551616.0f ? SIZE_MAX : (size_t)t);
        want = kAnim[l][cyc % n];
    }
    for (size_t i = 0; i < flat_names.size(); i++)
        if (flat_names[i] == want) return (int)i;
    return FLAT_MISSING;
}
int Scene::sprite_bitmap_id(const std::string &sprite, uint8_t frame, uint8_t rotation) const {
    std::string key = sprite + (char)('A' + frame);
    for (size_t i = 0; i < sprite_frame_keys.size(); i++)
        if (sprite_frame_keys[i] == key) {
            if (rotation > 7) return TEX_UNKNOWN;
            const SpriteFrameRec &f = sprite_frames[i];
            return f.rotate ? f.bitmap[rotation] : f.bitmap[0];
        }
    return TEX_UNKNOWN;
}

// Sprites::new restricted to one frame (src/graphics/sprites.rs:26-97), as far as the lump names tell: the lumps that hold (sprite,
// frame) in lump order with the rotation key each fills, whether the frame rotates, and the verdict — error is what add_sprite_frame
// throws, empty when the frame resolves.  Decodes nothing.
struct SpriteScan {
    struct Hit { int lump; uint8_t rot; bool mirror; };
    std::vector<Hit> hits;
    bool rotate = false;
    std::string error;
};
static SpriteScan scan_sprite_frame(const Builder &b, const std::string &sprite, uint8_t frame) {
    SpriteScan s;
    bool have[256] = {false};
    for (int idx = b.first_sprite; idx < b.last_sprite && s.error.empty(); idx++) {
        const std::string &nm = b.wad.dir[(size_t)idx].name;
        if (sprite.size() != 4 || nm.compare(0, 4, sprite) != 0) continue;
        if (nm.size() < 6) s.error = "sprite lump " + nm + " too short";
        else if (nm.size() == 7) s.error = "sprite lump " + nm + " malformed";
        else
            for (size_t at = 4; at < nm.size(); at += 2)
                if ((uint8_t)(nm[at] - 65) == frame) {
                    s.hits.push_back({idx, (uint8_t)(nm[at + 1] - 48), at > 4});
                    have[s.hits.back().rot] = true;
                }
    }
    if (!s.error.empty()) return s;
    int nkeys = 0;
    for (bool h : have) nkeys += h;
    s.rotate = nkeys != 1;
    if (nkeys == 0) s.error = "Unknown frame " + std::to_string(frame) + " for " + sprite + " (sprites.rs:104)";
    else if (nkeys == 1 && !have[0]) s.error = "sprite " + sprite + ": single rotation is not 0";
    else if (nkeys != 1 && nkeys != 8) s.error = "Got something other than 8 rotations for " + sprite;
    else if (nkeys == 8 && std::find(have + 1, have + 9, false) != have + 9) s.error = "sprite " + sprite + " misses a rotation";
    return s;
}
static int sprite_frame_index(const Scene &sc, const std::string &key) {
    for (size_t i = 0; i < sc.sprite_frame_keys.size(); i++)
        if (sc.sprite_frame_keys[i] == key) return (int)i;
    return -1;
}
// Whether add_sprite_frame would resolve (sprite, frame) as far as the lump names tell, decoding nothing.
static bool sprite_frame_resolves(const Builder &b, const std::string &sprite, uint8_t frame) {
    return sprite_frame_index(b.sc, sprite + (char)('A' + frame)) >= 0 || scan_sprite_frame(b, sprite, frame).error.empty();
}
static int add_sprite_frame(Builder &b, const std::string &sprite, uint8_t frame) {
    Scene &sc = b.sc;
    std::string key = sprite + (char)('A' + frame);
    const int known = sprite_frame_index(sc, key);
    if (known >= 0) return known;
    const SpriteScan scan = scan_sprite_frame(b, sprite, frame);
    if (!scan.error.empty()) throw LoadError(scan.error);
    int rot_bitmap[256];
    for (const SpriteScan::Hit &h : scan.hits) rot_bitmap[h.rot] = b.picture_bitmap(b.wad.dir[(size_t)h.lump].name, h.mirror);
    SpriteFrameRec f{};
    f.rotate = scan.rotate;
    for (int r = 0; r < 8; r++) f.bitmap[r] = rot_bitmap[f.rotate ? r + 1 : 0];
    sc.sprite_frames.push_back(f);
    sc.sprite_frame_keys.push_back(key);
    return (int)sc.sprite_frames.size() - 1;
}

void Scene::commit_new_frames(size_t frames_before) {
    if (sprite_frames.size() == frames_before) return;
    revision++;
    rebuild_fs_tables();
}

int Scene::find_or_add_sprite_frame(const std::string &sprite, uint8_t frame, std::string &err) {
    try {
        Builder b = Builder::resume(*this);
        const int id = add_sprite_frame(b, sprite, frame);
        commit_new_frames(0);                                                 // whether or not the frame is new, as ever (an id: there is a frame)
        return id;
    } catch (const std::exception &ex) {
        err = ex.what();
        return -1;
    }
}

// dg_scene_use_texture: Textures::get by the loader's rule (Builder::sidedef_texture); a new bitmap is appended, so no id moves.
int Scene::use_texture(const std::string &name, std::string &err) {
    if (name == "-") return TEX_NONE;
    try {
        Builder b = Builder::resume(*this);
        b.load_texture_defs();
        const size_t before = bitmaps.size();
        const int id = b.texture_bitmap(name);
        if (id < 0) { err = "Unknown texture " + name + " (Textures::get panics, textures.rs:158)"; return TEX_UNKNOWN; }
        if (bitmaps.size() != before) { revision++; rebuild_fs_tables(); }
        return id;
    } catch (const std::exception &ex) {
        err = ex.what();
        rebuild_fs_tables();
        return TEX_UNKNOWN;
    }
}

// dg_scene_use_picture: Pictures::get (pictures.rs:38-47) through the loader's picture_bitmap — the bitmap a sprite frame of that lump
// shares when one was loaded first.  A lump that fails to decode leaves nothing behind: add_bitmap runs after the decode.
int Scene::use_picture(const std::string &name, std::string &err) {
    try {
        Builder b = Builder::resume(*this);
        const size_t before = bitmaps.size();
        const int id = b.picture_bitmap(name, false);
        if (bitmaps.size() != before) { revision++; rebuild_fs_tables(); }
        const auto at = std::find(pictures.begin(), pictures.end(), id);
        if (at != pictures.end()) return (int)(at - pictures.begin());
        pictures.push_back(id);
        return (int)pictures.size() - 1;
    } catch (const std::exception &ex) {
        err = ex.what();
        return -1;
    }
}

// dg_scene_use_flat: Flats::get_animated by the loader's rule (the SECTORS loop of load_scene_from_wad): a member of an animated list
// is that list, every member loaded; any other name is its lump.  A list whose members are already one of Scene::anim is that one.
int Scene::use_flat(const std::string &name, std::string &err) {
    try {
        Builder b = Builder::resume(*this);
        const size_t before = flat_names.size();
        const bool sky = name.find("SKY") != std::string::npos;
        const int al = anim_list_of(name);
        int32_t h = -1;
        if (al >= 0) {
            AnimList a{};
            bool ok = true;
            while (kAnim[al][a.n]) { a.flat[a.n] = b.flat(kAnim[al][a.n]); ok &= a.flat[a.n] >= 0; a.n++; }
            if (ok) {
                size_t at = 0;
                while (at < anim.size() && !(anim[at].n == a.n && std::equal(a.flat, a.flat + a.n, anim[at].flat))) at++;
                if (at == anim.size()) anim.push_back(a);
                h = fs_flat_handle(-1, (int32_t)at, sky);
            }
        } else {
            const int id = b.flat(name);
            if (id >= 0) h = fs_flat_handle(id, -1, sky);
        }
        if (flat_names.size() != before || fs_anims.size() != anim.size()) { revision++; rebuild_fs_tables(); }
        if (h < 0) err = "Could not find flat lump " + name + " (Flat::new unwrap, flats.rs:117)";
        return h;
    } catch (const std::exception &ex) {
        err = ex.what();
        rebuild_fs_tables();
        return -1;
    }
}

// dg_scene_set_wall_effects: the live lists (members decoded through Textures::get, new bitmaps appended), then the per-seg table.
int Scene::set_wall_effects(uint32_t flags, std::string &err) {
    if (flags & ~(uint32_t)(DG_WALL_ANIMATE | DG_WALL_SCROLL)) { err = "unknown wall effect bits"; return DG_ERR_INVALID; }
    WallFx fx;
    fx.flags = flags;
    if (flags) {
        std::vector<int32_t> list_of_bitmap;                                  // bitmap id -> live list (-1: none)
        if (flags & DG_WALL_ANIMATE) {
            try {
                Builder b = Builder::resume(*this);
                b.load_texture_defs();
                for (const auto &l : kWallAnim) {
                    FsAnim a{};
                    bool live = true;
                    for (a.n = 0; a.n < 4 && l[a.n]; a.n++) {
                        a.flat[a.n] = b.texture_bitmap(l[a.n]);
                        live &= a.flat[a.n] >= 0;
                    }
                    if (!live) continue;
                    for (int k = 0; k < a.n; k++) {
                        if ((size_t)a.flat[k] >= list_of_bitmap.size()) list_of_bitmap.resize((size_t)a.flat[k] + 1, -1);
                        list_of_bitmap[(size_t)a.flat[k]] = (int32_t)fx.lists.size();
                    }
                    fx.lists.push_back(a);
                }
            } catch (const std::exception &ex) {
                err = ex.what();
                rebuild_fs_tables();                                          // (bitmaps decoded before the failure stay: ids never move)
                return DG_ERR_WAD;
            }
        }
        auto list_of = [&](int32_t tex) -> int8_t { return tex >= 0 && (size_t)tex < list_of_bitmap.size() ? (int8_t)list_of_bitmap[(size_t)tex] : (int8_t)-1; };
        std::vector<uint32_t> k(sidedefs.size(), 0);
        if (flags & DG_WALL_SCROLL)
            for (const LinedefRec &d : linedefs)
                if (d.special == kWallScrollSpecial && d.front >= 0) k[(size_t)d.front]++;
        fx.seg.resize(segs.size());
        for (size_t i = 0; i < segs.size(); i++) {
            const LinedefRec &ld = linedefs[(size_t)segs[i].linedef];
            const int sd = segs[i].direction ? ld.back : ld.front;            // the seg's own sidedef (fs_segs: segs.rs:358-362)
            FsSegFx &f = fx.seg[i];
            f = FsSegFx{0u, -1, -1, -1, 0};
            if (sd < 0) continue;
            const SidedefRec &r = sidedefs[(size_t)sd];
            f.scroll_k = k[(size_t)sd];
            f.anim_mid = list_of(r.middle); f.anim_low = list_of(r.lower); f.anim_up = list_of(r.upper);
        }
    }
    this->fx.wall = std::move(fx);
    rebuild_fs_tables();
    return DG_OK;
}
// dg_scene_set_light_effects: init_sector_thinkers (thinkers.rs:14-76) on the map as loaded — the WAD's levels, whatever
// set_sector_light has done since — with its ThreadRng draws replaced by lfx_draw; the flash and fire tables follow light_fx.h.
int Scene::set_light_effects(uint32_t flags, uint64_t seed, std::string &err) {
    if (flags & ~(uint32_t)DG_LIGHT_THINKERS) { err = "unknown light effect bits"; return DG_ERR_INVALID; }
    LightFx fx;
    fx.flags = flags; fx.seed = seed;
    if (flags) {
        auto min_surrounding = [&](size_t sector, int16_t mx) {          // find_min_surrounding_light, lights.rs:16-42
            int16_t lv = mx;
            for (const LinedefRec &d : linedefs) {
                if (d.front < 0 || d.back < 0) continue;
                const size_t fs = (size_t)sidedefs[(size_t)d.front].sector, bs = (size_t)sidedefs[(size_t)d.back].sector;
                if (fs == sector) lv = std::min(lv, wad_light[bs]);
                if (bs == sector) lv = std::min(lv, wad_light[fs]);
            }
            return lv;
        };
        fx.rec_of.assign(sectors.size(), -1);
        for (size_t i = 0; i < sectors.size(); i++) {
            const int16_t t = sectors[i].special;
            if (t != 1 && t != 2 && t != 3 && t != 4 && t != 8 && t != 12 && t != 13 && t != 17) continue;
            const int16_t mx = wad_light[i], surr = min_surrounding(i, mx);
            LfxRec r{(uint32_t)i, (uint8_t)t, 0, 0, surr, mx, 0};
            if (t == LFX_FIRE) r.min = lfx_wrap((uint32_t)(int32_t)surr + 16u);
            if (t == 2 || t == 3 || t == 4 || t == 12 || t == 13) {
                r.min = surr == mx ? (int16_t)0 : surr;
                r.dark = (t == 3 || t == 12) ? 35 : 15;           // SLOW_DARK / FAST_DARK
                r.c0 = (t == 12 || t == 13) ? 1 : (uint16_t)(1u + lfx_draw(seed, 2u, (uint32_t)i, 0u, 8u));
            }
            if (t == LFX_FLASH) {
                r.tab = (uint32_t)fx.tab.size();
                fx.tab.resize(fx.tab.size() + LFX_FLASH_WORDS);
                uint32_t *S = fx.tab.data() + r.tab, sum = 0;
                S[0] = 0;
                for (uint32_t k = 0; k < LFX_PERIOD_DRAWS; k++) {
                    sum += 1u + lfx_draw(seed, 1u, (uint32_t)i, k, (k & 1u) ? 7u : 64u);
                    if ((k + 1) % LFX_CHECKPOINT == 0) S[(k + 1) / LFX_CHECKPOINT] = sum;
                }
            }
            if (t == LFX_FIRE) {
                r.tab = (uint32_t)fx.tab.size();
                fx.tab.resize(fx.tab.size() + LFX_FIRE_WORDS, 0u);
                uint8_t *b = reinterpret_cast<uint8_t *>(fx.tab.data() + r.tab), *trans = b, *pmap = b + 20, *cp = b + 25;
                for (uint32_t x = 0; x < 5; x++)
                    for (uint32_t d = 0; d < 4; d++) {
                        const int16_t L = lfx_fire_level(r, x);
                        trans[x * 4 + d] = lfx_wrap((uint32_t)(int32_t)L - 16u * d) < r.min ? 4 : (uint8_t)d;
                    }
                for (uint32_t x0 = 0; x0 < 5; x0++) {
                    uint32_t x = x0;
                    for (uint32_t j = 1; j <= LFX_PERIOD_DRAWS; j++) {
                        if ((j - 1) % LFX_CHECKPOINT == 0) cp[x0 * 64 + (j - 1) / LFX_CHECKPOINT] = (uint8_t)x;
                        x = trans[x * 4 + lfx_draw(seed, 3u, (uint32_t)i, j % LFX_PERIOD_DRAWS, 4u)];
                    }
                    pmap[x0] = (uint8_t)x;
                }
            }
            fx.rec_of[i] = (int32_t)fx.recs.size();
            fx.recs.push_back(r);
        }
    }
    this->fx.light = std::move(fx);
    return DG_OK;
}

// dg_scene_set_mobj_thinkers: init_map_obj_thinkers (thinkers.rs:82-86) over the caller's tables.  Per start state in use — the spawn
// states of the things' types, and their death / xdeath states for the events — the chain mutate() walks (map_objects.rs:92-121),
// flattened for mobj_fx.h when it is live; the frames of live chains are decoded here (appended: ids never move).
int Scene::set_mobj_thinkers(uint32_t flags, const dg_state_rec *states, int n_states, const dg_mobj_info_rec *infos, int n_infos, std::string &err) {
    if (flags & ~(uint32_t)DG_MOBJ_THINKERS) { err = "unknown map-object thinker bits"; return DG_ERR_INVALID; }
    MobjFx fx;
    fx.flags = flags;
    if (!flags) { this->fx.mobj = std::move(fx); return DG_OK; }
    if (!states || n_states < 1 || n_states > MFX_MAX_STATES) { err = "state table: NULL or n_states outside [1, 65536]"; return DG_ERR_INVALID; }
    if (n_infos < 0 || (n_infos > 0 && !infos)) { err = "info table: NULL or n_infos negative"; return DG_ERR_INVALID; }
    for (int i = 0; i < n_states; i++) {
        if (states[i].tics < -1) { err = "state " + std::to_string(i) + ": tics below -1"; return DG_ERR_INVALID; }
        if (states[i].next_state < 0 || states[i].next_state >= n_states) { err = "state " + std::to_string(i) + ": next_state out of range"; return DG_ERR_INVALID; }
    }
    for (int i = 0; i < n_infos; i++)
        for (int32_t st : {infos[i].spawn_state, infos[i].death_state, infos[i].xdeath_state})
            if (st < 0 || st >= n_states) { err = "info row " + std::to_string(i) + ": state out of range"; return DG_ERR_INVALID; }

    const size_t frames_before = sprite_frames.size();
    try {
        Builder b = Builder::resume(*this);
        std::vector<int8_t> resolves((size_t)n_states, -1);                  // per state: -1 not asked yet, 0 / 1
        std::vector<int32_t> chain_of((size_t)n_states, -2), pos((size_t)n_states, -1);   // per start state: -2 not built yet, -1 not live, else its chain
        std::vector<int32_t> walk;
        auto sprite_of = [&](int32_t st) { return std::string(states[st].sprite, strnlen(states[st].sprite, 4)); };
        auto chain_from = [&](int32_t start) -> int32_t {
            if (chain_of[(size_t)start] != -2) return chain_of[(size_t)start];
            walk.clear();
            int32_t st = start, cycle_at = -1;                               // cycle_at: where in the walk the cycle starts
            for (;;) {
                pos[(size_t)st] = (int32_t)walk.size();
                walk.push_back(st);
                if (states[st].tics == -1) { cycle_at = (int32_t)walk.size() - 1; break; }     // for ever: a cycle of this one state
                st = states[st].next_state;
                if (pos[(size_t)st] >= 0) { cycle_at = pos[(size_t)st]; break; }
            }
            bool live = true;
            for (int32_t w : walk) {
                pos[(size_t)w] = -1;
                if (w == 0) continue;
                if (resolves[(size_t)w] < 0) resolves[(size_t)w] = sprite_frame_resolves(b, sprite_of(w), states[w].frame) ? 1 : 0;
                live &= resolves[(size_t)w] == 1;
            }
            int32_t id = -1;
            if (live) {
                MfxChain c{(uint32_t)fx.steps.size(), (uint32_t)cycle_at, (uint32_t)walk.size() - (uint32_t)cycle_at, 0u, 0u, 0u};
                uint32_t sum = 0;
                for (size_t k = 0; k < walk.size(); k++) {
                    const dg_state_rec &r = states[walk[k]];
                    if (k == (size_t)cycle_at) { c.prefix_total = sum; sum = 0; }
                    sum += r.tics < 1 ? 1u : (uint32_t)r.tics;
                    const int32_t val = mfx_encode(walk[k] == 0 ? -1 : add_sprite_frame(b, sprite_of(walk[k]), r.frame), r.full_bright);
                    fx.steps.push_back(MfxStep{sum, val});
                }
                c.period = sum;
                id = (int32_t)fx.chains.size();
                fx.chains.push_back(c);
            }
            return chain_of[(size_t)start] = id;
        };
        std::vector<int32_t> type_of_row((size_t)n_infos, -2);               // per info row: -2 not built yet, -1 not driven, else its MfxType
        fx.type_of.assign(mobjs.size(), -1);
        for (size_t i = 0; i < mobjs.size(); i++) {
            int row = -1;
            for (int k = 0; k < n_infos; k++)
                if (infos[k].doomednum == (int32_t)mobj_type[i]) row = k;    // a later row wins (HashMap::insert)
            if (row < 0) continue;
            if (type_of_row[(size_t)row] == -2) {
                type_of_row[(size_t)row] = -1;
                const int32_t spawn = chain_from(infos[row].spawn_state);
                if (spawn >= 0) {
                    MfxType t{{spawn, -1, -1, spawn}};
                    if (infos[row].death_state != 0) t.chain[DG_MOBJ_KILL] = chain_from(infos[row].death_state);
                    t.chain[DG_MOBJ_EXPLODE] = infos[row].xdeath_state != 0 ? chain_from(infos[row].xdeath_state) : t.chain[DG_MOBJ_KILL];
                    type_of_row[(size_t)row] = (int32_t)fx.types.size();
                    fx.types.push_back(t);
                }
            }
            fx.type_of[i] = type_of_row[(size_t)row];
            if (fx.type_of[i] >= 0) fx.driven.push_back((uint32_t)i);
        }
    } catch (const std::exception &ex) {
        err = ex.what();
        commit_new_frames(frames_before);                                    // (frames decoded before the failure stay: ids never move)
        return DG_ERR_WAD;
    }
    commit_new_frames(frames_before);
    this->fx.mobj = std::move(fx);
    return DG_OK;
}

int Scene::mobj_event(int what, float timestamp, std::string &err) {
    MobjFx &mobj_fx = fx.mobj;
    if (what == 0) { mobj_fx.events.clear(); return DG_OK; }
    if (!mobj_fx.flags) { err = "no map-object thinkers set"; return DG_ERR_INVALID; }
    if (what != DG_MOBJ_KILL && what != DG_MOBJ_EXPLODE && what != DG_MOBJ_RESPAWN) { err = "unknown map-object event"; return DG_ERR_INVALID; }
    const uint32_t tics = fs_tics(timestamp);
    if (!mobj_fx.events.empty() && tics < mobj_fx.events.back().tics) { err = "map-object events must not go back in time"; return DG_ERR_INVALID; }
    if (mobj_fx.events.size() >= MFX_MAX_EVENTS) { err = "more than 16 map-object events"; return DG_ERR_INVALID; }
    mobj_fx.events.push_back(MfxEvent{tics, (uint32_t)what});
    return DG_OK;
}

int Scene::wall_texture_id(const std::string &name, float timestamp) const {
    const int id = texture_id(name);
    const WallFx &wall_fx = fx.wall;
    if (id < 0 || !(wall_fx.flags & DG_WALL_ANIMATE)) return id;
    for (const FsAnim &a : wall_fx.lists)
        for (int k = 0; k < a.n; k++)
            if (a.flat[k] == id) return fs_resolve_flat(id, (int32_t)(&a - wall_fx.lists.data()), wall_fx.lists.data(), timestamp);
    return id;
}

void Scene::rebuild_fs_tables() {
    fs_sectors.resize(sectors.size());
    for (size_t i = 0; i < sectors.size(); i++) {
        const SectorRec &s = sectors[i];
        fs_sectors[i] = FsSector{s.floor_h, s.ceil_h, s.floor_flat, s.ceil_flat, s.floor_anim, s.ceil_anim, s.ceil_tex_sky};
    }
    fs_heights.resize(sectors.size());
    for (size_t i = 0; i < sectors.size(); i++) fs_heights[i] = FsHeights{sectors[i].floor_h, sectors[i].ceil_h};
    fs_flats.resize(sectors.size());
    // (the loader gives every animated sector a list of its own: a handle names the first of equal lists, as use_flat does)
    std::vector<int32_t> first_of(anim.size());
    {
        std::map<std::array<int32_t, 5>, int32_t> seen;
        for (size_t a = 0; a < anim.size(); a++) {
            std::array<int32_t, 5> key{anim[a].n, -1, -1, -1, -1};
            for (int k = 0; k < anim[a].n; k++) key[(size_t)k + 1] = anim[a].flat[k];
            first_of[a] = seen.emplace(key, (int32_t)a).first->second;
        }
    }
    const auto first_equal = [&](int32_t a) { return first_of[(size_t)a]; };
    for (size_t i = 0; i < sectors.size(); i++) {
        const SectorRec &s = sectors[i];
        fs_flats[i] = FsFlats{fs_flat_handle(s.floor_flat, s.floor_anim < 0 ? -1 : first_equal(s.floor_anim), s.floor_sky != 0),
                              fs_flat_handle(s.ceil_flat, s.ceil_anim < 0 ? -1 : first_equal(s.ceil_anim), s.ceil_tex_sky != 0)};
    }
    fs_anims.resize(anim.size());
    for (size_t i = 0; i < anim.size(); i++) {
        fs_anims[i].n = anim[i].n;
        for (int k = 0; k < 4; k++) fs_anims[i].flat[k] = anim[i].flat[k];
    }
    fs_bitmaps.resize(bitmaps.size());
    for (size_t i = 0; i < bitmaps.size(); i++)
        fs_bitmaps[i] = FsBitmap{bitmaps[i].texel_off, (int16_t)bitmaps[i].w, (int16_t)bitmaps[i].h, bitmaps[i].top_offset, (uint16_t)bitmaps[i].has_holes};
    fs_segs.resize(segs.size());
    fs_seg_side.assign(segs.size(), -1);
    for (size_t i = 0; i < segs.size(); i++) {
        const SegRec &sg = segs[i];
        const LinedefRec &ld = linedefs[(size_t)sg.linedef];
        const int fsd = sg.direction ? ld.back : ld.front, bsd = sg.direction ? ld.front : ld.back;   // segs.rs:358-362
        FsSeg f;
        std::memset(&f, 0, sizeof f);
        f.v1x = vx[(size_t)sg.v1]; f.v1y = vy[(size_t)sg.v1]; f.v2x = vx[(size_t)sg.v2]; f.v2y = vy[(size_t)sg.v2];
        f.front_sector = -1; f.back_sector = -1;
        f.tex_mid = f.tex_low = f.tex_up = TEX_NONE;
        if (fsd >= 0) {
            const SidedefRec &sd = sidedefs[(size_t)fsd];
            f.front_sector = sd.sector;
            fs_seg_side[i] = fsd;
            f.sd_xoff = sd.xoff; f.sd_yoff = sd.yoff;
            f.tex_mid = sd.middle; f.tex_low = sd.lower; f.tex_up = sd.upper;
            if (bsd >= 0) f.back_sector = sidedefs[(size_t)bsd].sector;
        }
        f.seg_offset = sg.offset;
        f.ld_flags = (uint16_t)ld.flags;
        fs_segs[i] = f;
    }
    // every seg belongs to at most one leaf (0xffff: to none — the walk never reaches it)
    fs_ok = !may_panic && subsectors.size() < 0xffffu && !nodes.empty() && !segs.empty();
    fs_seg_leaf.assign(segs.size(), (uint16_t)0xffffu);
    fs_leaf_first.resize(subsectors.size());
    for (size_t l = 0; l < subsectors.size(); l++) {
        fs_leaf_first[l] = (uint32_t)subsectors[l].first;
        for (int i = 0; i < subsectors[l].count; i++) {
            const size_t si = (size_t)(subsectors[l].first + i);
            if (subsectors[l].first < 0 || si >= segs.size() || fs_seg_leaf[si] != 0xffffu) { fs_ok = false; continue; }
            fs_seg_leaf[si] = (uint16_t)l;
        }
    }
    // the tree: depth-first from the root (the last node, map/mod.rs:57); a leaf reached twice or a path longer than 256 is not a tree
    fs_anc_off.assign(subsectors.size() + 1, 0);
    fs_anc.clear();
    if (fs_ok) {
        std::vector<std::vector<uint32_t>> chains(subsectors.size());
        std::vector<uint8_t> seen_leaf(subsectors.size(), 0), seen_node(nodes.size(), 0);
        std::vector<uint32_t> path;
        struct Item { int16_t child; uint32_t depth; uint32_t entry; };
        std::vector<Item> stack;
        const uint32_t root = (uint32_t)nodes.size() - 1;
        seen_node[root] = 1;
        stack.push_back(Item{nodes[root].rchild, 0, root});
        stack.push_back(Item{nodes[root].lchild, 0, root | 0x80000000u});
        while (!stack.empty() && fs_ok) {
            const Item it = stack.back();
            stack.pop_back();
            path.resize(it.depth);
            path.push_back(it.entry);
            if (path.size() > 256) { fs_ok = false; break; }
            if (it.child & (int16_t)0x8000) {
                const size_t l = (size_t)(it.child & 0x7fff);
                if (l >= subsectors.size() || seen_leaf[l]) { fs_ok = false; break; }
                seen_leaf[l] = 1;
                chains[l] = path;
            } else {
                const size_t n = (size_t)it.child;
                if (n >= nodes.size() || seen_node[n]) { fs_ok = false; break; }
                seen_node[n] = 1;
                stack.push_back(Item{nodes[n].rchild, (uint32_t)path.size(), (uint32_t)n});
                stack.push_back(Item{nodes[n].lchild, (uint32_t)path.size(), (uint32_t)n | 0x80000000u});
            }
        }
        for (size_t l = 0; l < subsectors.size() && fs_ok; l++)        // a leaf no path leads to: its segs are never visited
            if (!seen_leaf[l])
                for (int i = 0; i < subsectors[l].count; i++) fs_seg_leaf[(size_t)(subsectors[l].first + i)] = (uint16_t)0xffffu;
        std::vector<uint32_t> segs_left(nodes.size(), 0), segs_right(nodes.size(), 0);        // segs below each child of a node
        for (size_t l = 0; l < subsectors.size() && fs_ok; l++)
            for (uint32_t e : chains[l]) (e >> 31 ? segs_left : segs_right)[e & 0x7fffffffu] += (uint32_t)subsectors[l].count;
        for (size_t l = 0; l < subsectors.size() && fs_ok; l++) {
            fs_anc_off[l] = (uint32_t)fs_anc.size();
            for (uint32_t e : chains[l]) {
                const size_t n = e & 0x7fffffffu;
                fs_anc.push_back(FsAnc{nodes[n].x, nodes[n].y, nodes[n].dx, nodes[n].dy, (e >> 31 ? segs_right[n] : segs_left[n]) | (e & 0x80000000u)});
            }
        }
        fs_anc_off[subsectors.size()] = (uint32_t)fs_anc.size();
    }
    fs_mobjs.resize(mobjs.size());
    for (size_t i = 0; i < mobjs.size(); i++) fs_mobjs[i] = FsMobj{mobjs[i].x, mobjs[i].y, mobjs[i].angle, mobjs[i].sector};
}

Scene *load_scene_from_wad(const uint8_t *bytes, size_t len, const char *map_name, std::string &err) {
    Scene *sc = new Scene();
    try {
        sc->wad.assign(bytes, bytes + len);
        sc->map_name = map_name;
        Builder b(*sc);
        const Wad &w = b.wad;
        b.first_sprite = w.find("S_START");
        b.last_sprite = w.find("S_END");
        if (b.first_sprite < 0 || b.last_sprite < 0) throw LoadError("Could not find lump S_START / S_END (src/wad.rs:105-106)");

        enum { THINGS = 1, LINEDEFS, SIDEDEFS, VERTEXES, SEGS, SSECTORS, NODES, SECTORS };
        // VERTEXES (4 B)
        {
            const Lump &l = w.map_lump(map_name, VERTEXES);
            size_t n = l.size / 4;
            sc->vx.resize(n); sc->vy.resize(n);
            for (size_t i = 0; i < n; i++) { sc->vx[i] = (float)w.i16(l.off + i * 4); sc->vy[i] = (float)w.i16(l.off + i * 4 + 2); }
        }
        // SECTORS (26 B)
        std::vector<std::string> sec_floor, sec_ceil;
        {
            const Lump &l = w.map_lump(map_name, SECTORS);
            size_t n = l.size / 26;
            sc->sectors.resize(n);
            sc->wad_light.resize(n);
            for (size_t i = 0; i < n; i++) {
                size_t o = l.off + i * 26;
                SectorRec &s = sc->sectors[i];
                std::memset(&s, 0, sizeof s);
                s.floor_h = w.i16(o); s.ceil_h = w.i16(o + 2); s.light = w.i16(o + 20); s.special = w.i16(o + 22);
                sc->wad_light[i] = s.light;
                std::string fn = w.name8(o + 4), cn = w.name8(o + 12);
                s.floor_sky = fn.find("SKY") != std::string::npos;
                s.ceil_sky = s.ceil_tex_sky = cn.find("SKY") != std::string::npos;
                for (int side = 0; side < 2; side++) {
                    const std::string &nm = side ? cn : fn;
                    int al = anim_list_of(nm), fid = FLAT_MISSING, aidx = -1;
                    if (al >= 0) {
                        AnimList a{};
                        while (kAnim[al][a.n]) { a.flat[a.n] = b.flat(kAnim[al][a.n]); a.n++; }
                        sc->anim.push_back(a);
                        aidx = (int)sc->anim.size() - 1;
                    } else {
                        fid = b.flat(nm);
                    }
                    (side ? s.ceil_flat : s.floor_flat) = fid;
                    (side ? s.ceil_anim : s.floor_anim) = aidx;
                }
            }
        }
        // SIDEDEFS (30 B)
        b.load_texture_defs();
        {
            const Lump &l = w.map_lump(map_name, SIDEDEFS);
            size_t n = l.size / 30;
            sc->sidedefs.resize(n);
            for (size_t i = 0; i < n; i++) {
                size_t o = l.off + i * 30;
                SidedefRec &s = sc->sidedefs[i];
                s.xoff = (float)w.i16(o); s.yoff = (float)w.i16(o + 2);
                s.upper = b.sidedef_texture(w.name8(o + 4));
                s.lower = b.sidedef_texture(w.name8(o + 12));
                s.middle = b.sidedef_texture(w.name8(o + 20));
                int16_t sec = w.i16(o + 28);
                if (sec < 0 || (size_t)sec >= sc->sectors.size()) throw LoadError("sidedef references a missing sector");
                s.sector = sec;
            }
        }
        // LINEDEFS (14 B)
        {
            const Lump &l = w.map_lump(map_name, LINEDEFS);
            size_t n = l.size / 14;
            sc->linedefs.resize(n);
            for (size_t i = 0; i < n; i++) {
                size_t o = l.off + i * 14;
                LinedefRec &d = sc->linedefs[i];
                int16_t v1 = w.i16(o), v2 = w.i16(o + 2), f = w.i16(o + 10), bk = w.i16(o + 12);
                d.flags = w.i16(o + 4); d.special = w.i16(o + 6);
                if (v1 < 0 || v2 < 0 || (size_t)v1 >= sc->vx.size() || (size_t)v2 >= sc->vx.size()) throw LoadError("linedef references a missing vertex");
                if ((f != -1 && (f < 0 || (size_t)f >= sc->sidedefs.size())) || (bk != -1 && (bk < 0 || (size_t)bk >= sc->sidedefs.size())))
                    throw LoadError("linedef references a missing sidedef");
                d.v1 = v1; d.v2 = v2; d.front = f; d.back = bk;
            }
        }
        // SEGS (12 B)
        {
            const Lump &l = w.map_lump(map_name, SEGS);
            size_t n = l.size / 12;
            sc->segs.resize(n);
            for (size_t i = 0; i < n; i++) {
                size_t o = l.off + i * 12;
                SegRec &s = sc->segs[i];
                int16_t v1 = w.i16(o), v2 = w.i16(o + 2), ld = w.i16(o + 6);
                if (v1 < 0 || v2 < 0 || ld < 0 || (size_t)v1 >= sc->vx.size() || (size_t)v2 >= sc->vx.size() || (size_t)ld >= sc->linedefs.size())
                    throw LoadError("seg references a missing vertex/linedef");
                s.v1 = v1; s.v2 = v2; s.linedef = ld; s.direction = w.i16(o + 8) != 0; s.offset = w.i16(o + 10); s.pad = 0;
            }
        }
        // SSECTORS (4 B)
        {
            const Lump &l = w.map_lump(map_name, SSECTORS);
            size_t n = l.size / 4;
            sc->subsectors.resize(n);
            for (size_t i = 0; i < n; i++) {
                int16_t cnt = w.i16(l.off + i * 4), first = w.i16(l.off + i * 4 + 2);
                if (cnt < 0 || first < 0 || (size_t)(first + cnt) > sc->segs.size()) throw LoadError("subsector references missing segs");
                sc->subsectors[i] = SubSectorRec{first, cnt};
            }
        }
        // NODES (28 B); children precede parents, root = last (src/map/nodes.rs:45-83, src/map/mod.rs:57)
        {
            const Lump &l = w.map_lump(map_name, NODES);
            size_t n = l.size / 28;
            if (n == 0) throw LoadError("map has no BSP nodes");
            sc->nodes.resize(n);
            for (size_t i = 0; i < n; i++) {
                size_t o = l.off + i * 28;
                NodeRec &d = sc->nodes[i];
                d.x = (float)w.i16(o); d.y = (float)w.i16(o + 2); d.dx = (float)w.i16(o + 4); d.dy = (float)w.i16(o + 6);
                d.rchild = w.i16(o + 24); d.lchild = w.i16(o + 26);
                for (int16_t ch : {d.rchild, d.lchild}) {
                    size_t idx = (size_t)(ch & 0x7fff);
                    if (ch & (int16_t)0x8000) { if (idx >= sc->subsectors.size()) throw LoadError("node references a missing subsector"); }
                    else if (idx >= i) throw LoadError("node references a node that is not loaded yet");
                }
            }
        }
        // Bounding boxes of the subtrees (children precede parents, so one ascending pass suffices) and whether any record
        // could make the reference panic when its seg is processed (then no seg may be skipped unseen, frontend.cpp).
        {
            auto grow = [](float *bb, float x, float y) { bb[0] = std::min(bb[0], x); bb[1] = std::min(bb[1], y); bb[2] = std::max(bb[2], x); bb[3] = std::max(bb[3], y); };
            for (size_t i = 0; i < sc->nodes.size(); i++) {
                NodeRec &d = sc->nodes[i];
                const int16_t child[2] = {d.rchild, d.lchild};
                for (int side = 0; side < 2; side++) {
                    float *bb = d.bb[side];
                    bb[0] = bb[1] = 3.0e38f; bb[2] = bb[3] = -3.0e38f;
                    const size_t idx = (size_t)(child[side] & 0x7fff);
                    if (child[side] & (int16_t)0x8000) {
                        const SubSectorRec &ss = sc->subsectors[idx];
                        for (int k = 0; k < ss.count; k++) {
                            const SegRec &sg = sc->segs[(size_t)(ss.first + k)];
                            grow(bb, sc->vx[(size_t)sg.v1], sc->vy[(size_t)sg.v1]);
                            grow(bb, sc->vx[(size_t)sg.v2], sc->vy[(size_t)sg.v2]);
                        }
                    } else {
                        for (int s2 = 0; s2 < 2; s2++) { grow(bb, sc->nodes[idx].bb[s2][0], sc->nodes[idx].bb[s2][1]); grow(bb, sc->nodes[idx].bb[s2][2], sc->nodes[idx].bb[s2][3]); }
                    }
                }
            }
            sc->may_panic = false;
            for (const SidedefRec &sd : sc->sidedefs) sc->may_panic |= sd.upper == TEX_UNKNOWN || sd.lower == TEX_UNKNOWN || sd.middle == TEX_UNKNOWN;
            for (const SectorRec &se : sc->sectors) sc->may_panic |= (se.floor_anim < 0 && se.floor_flat < 0) || (se.ceil_anim < 0 && se.ceil_flat < 0);
            for (const AnimList &a : sc->anim)
                for (int k = 0; k < a.n; k++) sc->may_panic |= a.flat[k] < 0;
        }
        // Palette (first 768 bytes of PLAYPAL)
        {
            int pi = w.find("PLAYPAL");
            if (pi < 0) throw LoadError("Could not find lump PLAYPAL");
            w.need(w.dir[(size_t)pi].off, 768, "PLAYPAL");
            std::memcpy(sc->palette, &sc->wad[w.dir[(size_t)pi].off], 768);
        }
        sc->sky_bitmap = b.texture_bitmap(sky_name_for_map(map_name));
        if (sc->sky_bitmap < 0) throw LoadError("Unknown texture for the sky (src/game.rs:199-227)");
        // THINGS (10 B) -> player start + map objects in spawn state
        {
            const Lump &l = w.map_lump(map_name, THINGS);
            size_t n = l.size / 10;
            for (size_t i = 0; i < n; i++) {
                size_t o = l.off + i * 10;
                float x = (float)w.i16(o), y = (float)w.i16(o + 2);
                float angle = (float)w.i16(o + 4) * (kPi / 180.0f);   // f32::to_radians (src/map/things.rs:36)
                int16_t type = w.i16(o + 6);
                if (type == 1 && !sc->has_start) { sc->start_x = x; sc->start_y = y; sc->start_angle = angle; sc->has_start = true; }
                if ((type >= 1 && type <= 4) || type == 11) continue;                 // map_objects.rs:31-36
                const SpawnRow *row = nullptr;
                for (const SpawnRow &r : kSpawn)
                    if (r.id == type) row = &r;
                if (!row) throw LoadError("thing type " + std::to_string(type) + " has no MapObjectInfo (reference unwrap panic)");
                MapObjectRec m{};
                m.x = x; m.y = y; m.angle = angle;
                m.full_bright = row->full_bright;
                m.sprite_frame = row->is_null ? -1 : add_sprite_frame(b, row->sprite, row->frame);
                m.sector = sc->sector_from_vertex(x, y);
                sc->mobjs.push_back(m);
                sc->mobj_type.push_back(type);
            }
        }
        for (const LinedefRec &d : sc->linedefs)
            for (int32_t v : {d.v1, d.v2}) {
                const float x = sc->vx[(size_t)v], y = sc->vy[(size_t)v];
                sc->map_left = std::min(sc->map_left, x); sc->map_right = std::max(sc->map_right, x);
                sc->map_top = std::min(sc->map_top, y); sc->map_bottom = std::max(sc->map_bottom, y);
            }
        sc->rebuild_fs_tables();
        sc->build_walk_tables();
        return sc;
    } catch (const std::exception &ex) {
        err = ex.what();
        delete sc;
        return nullptr;
    }
}

}  // namespace dg

namespace dg {

// transform_vertex_to_point_for_map (src/game.rs:229-243), every operation in f32 in the reference's order (no FMA: -ffp-contract=off)
namespace {
struct MapXform {
    float left, top, xs, ys, sw, sh;
    void point(float vx, float vy, int32_t &X, int32_t &Y) const {
        const float b = 20.0f;
        X = f32_as_i32(b + ((vx - left) * sw) / xs);
        Y = f32_as_i32(((b + sh) - 1.0f) - ((vy - top) * sh) / ys);
    }
};
MapXform map_xform(const Scene &sc, int W, int H) {
    return MapXform{sc.map_left, sc.map_top, sc.map_right - sc.map_left, sc.map_bottom - sc.map_top, (float)(W - 40), (float)(H - 40)};
}
constexpr uint32_t kMapRed = 0x0000ffu, kMapYellow = 0x00ffffu;   // Color::RGB(255, 0, 0) / (255, 255, 0) as r | g << 8 | b << 16
}  // namespace

int map_arrow_lines(const Scene &sc, int W, int H, const dg_view &view, dg_map_line out[3], std::string &err) {
    if (W < 40 || H < 40 || W > 16384 || H > 16384) { err = "map frames need width and height in [40, 16384]"; return DG_ERR_INVALID; }
    const MapXform t = map_xform(sc, W, H);
    // draw_map_player, game.rs:287-309: Vertex::rotate (vertexes.rs:20-25) evaluated literally, 0.0 products included
    const float PI = 3.14159265358979323846f;                                  // std::f32::consts::PI
    const float a = view.angle, len = (float)W / 16.0f, alen = (float)W / 32.0f;
    const float zero = 0.0f;
    const float c = view.cos_a, s = view.sin_a;
    const float px = view.x, py = view.y;
    const float ex = px + (len * c - zero * s), ey = py + (zero * c + len * s);
    const float ar = (a - PI) - PI / 4.0f, al = (a - PI) + PI / 4.0f;
    const float cr = cosf(ar), sr = sinf(ar), cl = cosf(al), sl = sinf(al);
    const float rx = ex + (alen * cr - zero * sr), ry = ey + (zero * cr + alen * sr);
    const float lx = ex + (alen * cl - zero * sl), ly = ey + (zero * cl + alen * sl);
    int32_t P[4][2];
    t.point(px, py, P[0][0], P[0][1]);
    t.point(ex, ey, P[1][0], P[1][1]);
    t.point(rx, ry, P[2][0], P[2][1]);
    t.point(lx, ly, P[3][0], P[3][1]);
    for (auto &p : P)
        for (int32_t v : p)
            if (v < -(1 << 24) || v > (1 << 24)) {
                err = "the player arrow lands beyond +-2^24 pixels of the map frame (out of contract: SDL's int -> float -> int round trip is not exact there)";
                return DG_ERR_INVALID;
            }
    out[0] = dg_map_line{P[0][0], P[0][1], P[1][0], P[1][1], kMapYellow};
    out[1] = dg_map_line{P[2][0], P[2][1], P[1][0], P[1][1], kMapYellow};
    out[2] = dg_map_line{P[3][0], P[3][1], P[1][0], P[1][1], kMapYellow};
    return DG_OK;
}

int map_frame_lines(const Scene &sc, int W, int H, const dg_view *view, std::vector<dg_map_line> &out, std::string &err) {
    out.clear();
    if (W < 40 || H < 40 || W > 16384 || H > 16384) { err = "map frames need width and height in [40, 16384]"; return DG_ERR_INVALID; }
    dg_map_line arrow[3];
    if (view) {
        const int rc = map_arrow_lines(sc, W, H, *view, arrow, err);
        if (rc) return rc;
    }
    const MapXform t = map_xform(sc, W, H);
    for (const LinedefRec &d : sc.linedefs) {                                  // draw_map_linedefs, game.rs:245-262
        if (d.flags & 128) continue;                                           // DONTDRAW
        dg_map_line l;
        t.point(sc.vx[(size_t)d.v1], sc.vy[(size_t)d.v1], l.x0, l.y0);
        t.point(sc.vx[(size_t)d.v2], sc.vy[(size_t)d.v2], l.x1, l.y1);
        l.rgb = (d.flags & 4) ? kMapYellow : kMapRed;                          // TWOSIDED
        out.push_back(l);
    }
    if (view) out.insert(out.end(), arrow, arrow + 3);
    return DG_OK;
}

}  // namespace dg
