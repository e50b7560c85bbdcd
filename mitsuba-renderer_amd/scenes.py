"""Procedural scene descriptions for the configurations of SURVEY.md section 8(d).

A description is what Mitsuba's XML loader would hand to Scene::addChild: plain
triangle meshes (TriMesh ctor, include/mitsuba/render/trimesh.h:52-56), BSDF and
luminaire property blocks and a lookAt camera.  Nothing here is on the hot path;
flattening (normals, CDFs, TriAccel, kd-tree) happens in mtsgpu_flatten().
All arithmetic is float32 so the arrays are identical on every host."""
import ctypes as C
import numpy as np
from . import abi

F = np.float32


class _VertexColors:
    """the `vertexcolors` texture (src/textures/vertexcolors.cpp): getValue(its) = its.color"""

    def __repr__(self):
        return "VERTEX_COLORS"


# pass this where a BSDF constructor of SceneDescription takes a reflectance or transmittance: the slot then takes the
# colour interpolated from the mesh's per-vertex colours, and the block holds the texture's getAverage() = getMaximum() = 1
VERTEX_COLORS = _VertexColors()


class _UvTexture:
    """Texture2D (src/librender/texture.cpp:43-52): uv' = uv * (uscale, vscale) + (uoffset, voffset); brightColor and
    darkColor as a grey level or an RGB triple"""
    kind = -1

    def __init__(self, bright=0.4, dark=0.2, uoffset=0.0, voffset=0.0, uscale=1.0, vscale=1.0, line_width=0.01):
        self.bright = np.broadcast_to(np.asarray(bright, dtype=np.float32), (3,)).copy()
        self.dark = np.broadcast_to(np.asarray(dark, dtype=np.float32), (3,)).copy()
        self.uoffset, self.voffset, self.uscale, self.vscale = F(uoffset), F(voffset), F(uscale), F(vscale)
        self.line_width = F(line_width)

    def maximum(self):
        return self.bright.copy()

    def descriptor(self):
        """the twelve words of mtsgpu_uv_texture"""
        return abi.UvTexture(self.kind, self.uoffset, self.voffset, self.uscale, self.vscale, (C.c_float * 3)(*self.bright),
                             (C.c_float * 3)(*self.dark), self.line_width)


class Checkerboard(_UvTexture):
    """the `checkerboard` texture (src/textures/checkerboard.cpp); pass it where a BSDF constructor of SceneDescription takes a
    reflectance or transmittance.  The block then holds getAverage() = darkColor * .5f (sic, :66-68)"""
    kind = abi.TEX_CHECKERBOARD

    def __init__(self, bright=0.4, dark=0.2, uoffset=0.0, voffset=0.0, uscale=1.0, vscale=1.0):
        _UvTexture.__init__(self, bright, dark, uoffset, voffset, uscale, vscale)

    def average(self):
        return self.dark * F(0.5)


class GridTexture(_UvTexture):
    """the `gridtexture` texture (src/textures/gridtexture.cpp): dark lines of half-width lineWidth on the integer uv'
    lines.  The block holds getAverage() = brightColor (:79-81)"""
    kind = abi.TEX_GRID

    def average(self):
        return self.bright.copy()


WRAP_MODES = {"repeat": abi.WRAP_REPEAT, "clamp": abi.WRAP_CLAMP, "black": abi.WRAP_BLACK, "white": abi.WRAP_WHITE}


class BitmapTexture(_UvTexture):
    """the `ldrtexture` texture (src/textures/ldrtexture.cpp) with filterType = "none": the texel that holds uv', no
    filtering; pass it where a BSDF constructor of SceneDescription takes a reflectance or transmittance.  texels: [height]
    [width][3] linear RGB float32, what the MIPMap's level 0 holds -- or pixels: the decoded file as a uint8 array [height]
    [width] (8 bpp), [height][width][2] (16), [..][3] (24) or [..][4] (32), converted with `gamma` (-1 = sRGB) by
    mtsgpu_ldr_texels, the restatement of LDRTexture::initializeFrom.  wrap: repeat, clamp, black or white.  Two textures that
    are given the same texels array and wrap mode share one bitmap on the device."""
    kind = abi.TEX_BITMAP

    def __init__(self, texels=None, pixels=None, gamma=-1.0, wrap="repeat", uoffset=0.0, voffset=0.0, uscale=1.0, vscale=1.0):
        _UvTexture.__init__(self, 0.0, 0.0, uoffset, voffset, uscale, vscale)
        if (texels is None) == (pixels is None):
            raise ValueError("BitmapTexture: give texels or pixels")
        if pixels is not None:
            from . import ldr_texels
            texels = ldr_texels(pixels, gamma)
        if not (isinstance(texels, np.ndarray) and texels.dtype == np.float32 and texels.flags["C_CONTIGUOUS"]):
            texels = np.ascontiguousarray(texels, dtype=np.float32)
        if texels.ndim != 3 or texels.shape[2] != 3 or texels.size == 0:
            raise ValueError("BitmapTexture: texels are [height][width][3]")
        self.texels = texels
        self.height, self.width = texels.shape[:2]
        self.wrap_name = wrap
        self.wrap = WRAP_MODES[wrap]

    def average(self):
        """m_average = triangle(levels - 1, 0, 0) with one level (ldrtexture.cpp:206): getTexel(0, 0, 0), and column 0 counts as
        out of range there (mipmap.cpp:207) -- texel (0, 0) under repeat and clamp, the constant under black and white"""
        if self.wrap == abi.WRAP_BLACK:
            return np.zeros(3, dtype=np.float32)
        if self.wrap == abi.WRAP_WHITE:
            return np.ones(3, dtype=np.float32)
        return self.texels[0, 0].copy()

    def maximum(self):
        """MIPMap::getMaximum (mipmap.cpp:137-154): per channel over the texels, at least 1 under white"""
        m = self.texels.reshape(-1, 3).max(axis=0)
        return np.maximum(m, F(1.0)) if self.wrap == abi.WRAP_WHITE else m

    def descriptor(self):
        """the twelve words of mtsgpu_uv_texture: kind and Texture2D's four floats count, the library fills the rest"""
        return abi.UvTexture(self.kind, self.uoffset, self.voffset, self.uscale, self.vscale)

    def bitmap(self):
        """mtsgpu_bitmap over this texture's texels (which must outlive it)"""
        return abi.Bitmap(self.width, self.height, self.wrap, 0, abi.ptr(self.texels, abi.f32p))


def _slot_average(v):
    """what a texture-typed argument of a BSDF leaves in the block: Texture::getAverage() (a constant: itself)"""
    return v.average() if isinstance(v, _UvTexture) else F(1.0) if v is VERTEX_COLORS else v


def _slot_maximum(v):
    """Texture::getMaximum(), which verifyEnergyConservation reads (phong.cpp:81-90, ward.cpp)"""
    return v.maximum() if isinstance(v, _UvTexture) else F(1.0) if v is VERTEX_COLORS else v


def _rgb(v):
    return [F(x) for x in np.broadcast_to(np.asarray(v, dtype=np.float32), (3,))]


class Yarn:
    """one `Yarn` of a weave pattern (irawan.h:41-73): type "warp" / "weft" (or abi.YARN_*), angles in radians"""

    def __init__(self, type="warp", psi=0.0, umax=0.0, kappa=0.0, width=0.0, length=0.0, centerU=0.0, centerV=0.0, kd=0.0, ks=0.0):
        self.type = {"warp": abi.YARN_WARP, "weft": abi.YARN_WEFT}.get(type, type)
        self.psi, self.umax, self.kappa, self.width, self.length = F(psi), F(umax), F(kappa), F(width), F(length)
        self.centerU, self.centerV = F(centerU), F(centerV)
        self.kd, self.ks = np.float32(_rgb(kd)), np.float32(_rgb(ks))

    def __eq__(self, o):
        return isinstance(o, Yarn) and all(np.array_equal(np.float32(getattr(self, n)), np.float32(getattr(o, n))) for n in
                                           ("type", "psi", "umax", "kappa", "width", "length", "centerU", "centerV", "kd", "ks"))


class Weave:
    """a `WeavePattern` (irawan.h:130-165) with the four properties IrawanClothBRDF keeps next to it: the scalars of
    abi.WEAVE_SCALARS, pattern (1-based yarn ids, row by row) and yarns (Yarn objects)"""

    def __init__(self, name="", pattern=(), yarns=(), **scalars):
        self.name = name
        self.pattern = [int(p) for p in pattern]
        self.yarns = list(yarns)
        for n in abi.WEAVE_SCALARS:
            v = scalars.pop(n, 1.0 if n in ("repeatU", "repeatV", "kdMultiplier", "ksMultiplier") else 0)
            setattr(self, n, int(v) if n in ("tileWidth", "tileHeight") else F(v))
        if scalars:
            raise ValueError("Weave: unknown parameter(s) %s" % ", ".join(sorted(scalars)))

    def replace(self, **scalars):
        """a copy with some scalars replaced"""
        w = Weave(self.name, self.pattern, self.yarns, **{n: getattr(self, n) for n in abi.WEAVE_SCALARS})
        for n, v in scalars.items():
            if n not in abi.WEAVE_SCALARS:
                raise ValueError("Weave: unknown parameter %s" % n)
            setattr(w, n, int(v) if n in ("tileWidth", "tileHeight") else F(v))
        return w

    def __eq__(self, o):
        return isinstance(o, Weave) and self.name == o.name and self.pattern == o.pattern and self.yarns == o.yarns \
            and all(getattr(self, n) == getattr(o, n) for n in abi.WEAVE_SCALARS)


def load_weave(text, params=None):
    """The weave-file grammar of the reference (irawan.h:268-377): `weave { name = "...", key = value, ..., pattern { 1, 2, ... },
    yarn { type = warp | weft, key = value, ..., kd = {r, g, b} | $name, ks = ... }, ... }` with /* */ comments; a value is a
    number or $name, substituted from `params` (a spectrum parameter: a grey level or an RGB triple).  psi, umax and the four d*UmaxOverD* are given in degrees and kept in radians
    (value * M_PI / 180 in binary64, rounded to binary32, as the grammar's actions compute it).  -> Weave.  ValueError with the reason otherwise."""
    import re
    params = params or {}
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    tokens = re.findall(r'"[^"]*"|\$[A-Za-z_][A-Za-z_0-9]*|[A-Za-z_][A-Za-z_0-9]*|[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?|[{}=,]|\S', text)
    pos = [0]

    def peek():
        return tokens[pos[0]] if pos[0] < len(tokens) else None

    def take(expect=None):
        t = peek()
        if t is None or (expect is not None and t != expect):
            raise ValueError("load_weave: expected %s, found %s (token %d)" % (expect or "a token", "the end" if t is None else repr(t), pos[0]))
        pos[0] += 1
        return t

    def number():
        t = take()
        if t.startswith("$"):
            if t[1:] not in params:
                raise ValueError("load_weave: parameter %s is not given" % t)
            return F(params[t[1:]])
        try:
            return F(float(t))
        except ValueError:
            raise ValueError("load_weave: expected a number, found %r (token %d)" % (t, pos[0] - 1))

    def spectrum():
        if peek() == "{":
            take("{"); r = number(); take(","); g = number(); take(","); b = number(); take("}")
            return [r, g, b]
        t = take()
        if not t.startswith("$"):
            raise ValueError("load_weave: a spectrum is {r, g, b} or a $parameter, found %r" % t)
        if t[1:] not in params:
            raise ValueError("load_weave: parameter %s is not given" % t)
        return _rgb(params[t[1:]])

    deg = lambda v: F(float(v) * np.pi / 180)           # _1 * M_PI / 180: binary64, stored in a Float
    weave_floats = ("alpha", "beta", "ss", "hWidth", "warpArea", "weftArea", "fineness", "period")
    weave_degrees = ("dWarpUmaxOverDWarp", "dWarpUmaxOverDWeft", "dWeftUmaxOverDWarp", "dWeftUmaxOverDWeft")
    yarn_floats = ("kappa", "width", "length", "centerU", "centerV")

    def yarn():
        take("{")
        kw = {}
        while peek() != "}":
            key = take()
            take("=")
            if key == "type":
                t = take()
                if t not in ("warp", "weft"):
                    raise ValueError("load_weave: yarn type %r is neither warp nor weft" % t)
                kw["type"] = t
            elif key in ("psi", "umax"):
                kw[key] = deg(number())
            elif key in yarn_floats:
                kw[key] = number()
            elif key in ("kd", "ks"):
                kw[key] = spectrum()
            else:
                raise ValueError("load_weave: unknown yarn parameter %r" % key)
            if peek() == ",":
                take(",")
        take("}")
        return Yarn(**kw)

    take("weave"); take("{")
    name, scalars, pattern, yarns = "", {}, [], []
    while peek() != "}":
        key = take()
        if key == "pattern":
            take("{")
            while peek() != "}":
                t = take()
                if not t.isdigit():
                    raise ValueError("load_weave: pattern entry %r is not an unsigned integer" % t)
                pattern.append(int(t))
                if peek() == ",":
                    take(",")
            take("}")
        elif key == "yarn":
            yarns.append(yarn())
        else:
            take("=")
            if key == "name":
                t = take()
                if not t.startswith('"'):
                    raise ValueError("load_weave: the name is a quoted string, found %r" % t)
                name = t[1:-1]
            elif key in ("tileWidth", "tileHeight"):
                t = take()
                if not t.isdigit():
                    raise ValueError("load_weave: %s = %r is not an unsigned integer" % (key, t))
                scalars[key] = int(t)
            elif key in weave_floats:
                scalars[key] = number()
            elif key in weave_degrees:
                scalars[key] = deg(number())
            else:
                raise ValueError("load_weave: unknown weave parameter %r" % key)
        if peek() == ",":
            take(",")
    take("}")
    if peek() is not None:
        raise ValueError("load_weave: text after the weave: %r" % peek())
    return Weave(name, pattern, yarns, **scalars)


class MeshDesc:
    def __init__(self, positions, triangles, bsdf=-1, lum=-1, face_normals=True, normals=None, name="", colors=None, texcoords=None):
        self.positions = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        self.triangles = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
        self.normals = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        # per-vertex colours of a TriMesh (trimesh.h:121-126), [n_verts][3] linear RGB, or None
        self.colors = None if colors is None else np.ascontiguousarray(colors, dtype=np.float32).reshape(-1, 3)
        if self.colors is not None and self.colors.shape[0] != self.positions.shape[0]:
            raise ValueError("one colour per vertex: %d colours, %d vertices" % (self.colors.shape[0], self.positions.shape[0]))
        # texture coordinates of a TriMesh (m_texcoords), [n_verts][2], or None
        self.texcoords = None if texcoords is None else np.ascontiguousarray(texcoords, dtype=np.float32).reshape(-1, 2)
        if self.texcoords is not None and self.texcoords.shape[0] != self.positions.shape[0]:
            raise ValueError("one texcoord per vertex: %d texcoords, %d vertices" % (self.texcoords.shape[0], self.positions.shape[0]))
        self.bsdf, self.lum, self.face_normals, self.name = int(bsdf), int(lum), bool(face_normals), name
        self.shape_type, self.sphere = abi.SHAPE_TRIMESH, None


class SphereDesc(MeshDesc):
    """<shape type="sphere"> with `center` and `radius` (src/shapes/sphere.cpp:44-47): one kd-tree primitive"""

    def __init__(self, center, radius, bsdf=-1, lum=-1, inverted=False, name="sphere"):
        MeshDesc.__init__(self, np.zeros((0, 3)), np.zeros((0, 3), dtype=np.uint32), bsdf, lum, True, None, name)
        self.shape_type = abi.SHAPE_SPHERE
        self.sphere = (tuple(float(F(v)) for v in center), float(F(radius)), bool(inverted))


class CylinderDesc(MeshDesc):
    """<shape type="cylinder"> (src/shapes/cylinder.cpp:34-64) with `p1`, `p2` and `radius`, or with a `toWorld` from the unit
    cylinder (4 x 4, last row 0 0 0 1): one kd-tree primitive.  No area luminaire: the reference cannot render one either."""

    def __init__(self, p1=None, p2=None, radius=None, to_world=None, bsdf=-1, lum=-1, name="cylinder"):
        MeshDesc.__init__(self, np.zeros((0, 3)), np.zeros((0, 3), dtype=np.uint32), bsdf, lum, True, None, name)
        self.shape_type = abi.SHAPE_CYLINDER
        if to_world is not None:
            if p1 is not None or p2 is not None or radius is not None:
                raise ValueError("a cylinder takes p1, p2 and radius, or to_world")
            self.cylinder = (abi.CYLINDER_TOWORLD, (0.0,) * 3, (0.0,) * 3, 0.0, tuple(float(v) for v in np.asarray(to_world, dtype=np.float32).reshape(16)))
        else:
            if p1 is None or p2 is None or radius is None:
                raise ValueError("a cylinder takes p1, p2 and radius, or to_world")
            self.cylinder = (abi.CYLINDER_POINTS, tuple(float(F(v)) for v in p1), tuple(float(F(v)) for v in p2), float(F(radius)), (0.0,) * 16)

    def to_struct(self):
        form, p1, p2, radius, tw = self.cylinder
        return abi.Cylinder(form, (C.c_float * 3)(*p1), (C.c_float * 3)(*p2), radius, (C.c_float * 16)(*tw))


class SceneDescription:
    """meshes + BSDF blocks + luminaires + camera (+ integrator defaults for the config)"""

    def __init__(self, name):
        self.name = name
        self.meshes = []
        self.bsdf_type = []
        self.bsdf_params = []
        self.bsdf_color_slots = []  # per BSDF: bit s = its s-th texture slot takes its.color (include/mtsgpu.h)
        self.textures = []          # the Checkerboard / GridTexture / BitmapTexture objects in use (what mtsgpu_set_uv_textures takes)
        self.bsdf_slot_texture = [] # per BSDF: [index into textures or -1] for its two texture slots
        self._slot_textures = ()
        self.bsdf_masks = {}        # BSDF index -> the opacity of the mask around it: an RGB triple or an entry of textures
        self.bsdf_snow = {}         # BSDF index -> (abi.SNOW_*, the raw parameters its configure call takes)
        self.weaves = []            # the Weave objects of the cloth BSDFs
        self.bsdf_weave = {}        # BSDF index -> index into weaves
        self.lum_type = []
        self.lum_params = []
        self.camera = dict(origin=(0.0, 1.0, 3.4), target=(0.0, 1.0, 0.0), up=(0.0, 1.0, 0.0), fov=39.3)
        self.max_depth = -1
        self.rr_depth = 10
        self.env_bitmap = None      # [H][W][3] float32 of the envmap luminaire

    # --- property blocks --------------------------------------------------
    def add_bsdf(self, btype, params, color_slots=0):
        p = np.zeros(abi.BSDF_NPARAMS, dtype=np.float32)
        p[:len(params)] = np.asarray(params, dtype=np.float32)
        self.bsdf_type.append(int(btype))
        self.bsdf_params.append(p)
        self.bsdf_color_slots.append(int(color_slots))
        row = [-1, -1]
        for s, t in enumerate(self._slot_textures):        # left by _textured() for the constructor that called it
            if t is not None:
                if not any(t is u for u in self.textures):
                    self.textures.append(t)
                row[s] = [i for i, u in enumerate(self.textures) if u is t][0]
        self._slot_textures = ()
        self.bsdf_slot_texture.append(row)
        return len(self.bsdf_type) - 1

    def _textured(self, *values):
        """VERTEX_COLORS among the texture-typed arguments of a BSDF -> (the values with 1.0 in its place: the texture's
        getAverage() / getMaximum(), vertexcolors.cpp:49-55; the slot mask, bit s for the s-th argument).  A Checkerboard or
        GridTexture is replaced by its getAverage(), an RGB triple, and noted for add_bsdf, which fills bsdf_slot_texture"""
        mask = sum(1 << s for s, v in enumerate(values) if v is VERTEX_COLORS)
        self._slot_textures = tuple(v if isinstance(v, _UvTexture) else None for v in values)
        return [1.0 if v is VERTEX_COLORS else _slot_average(v) for v in values], mask

    def lambertian(self, r, g=None, b=None):
        (r,), slots = self._textured(r)
        if np.ndim(r):
            r, g, b = r
        g = r if g is None else g
        b = r if b is None else b
        return self.add_bsdf(abi.BSDF_LAMBERTIAN, [r, g, b], slots)

    def dielectric(self, int_ior=1.5046, ext_ior=1.0, refl=1.0, trans=1.0):
        (refl, trans), slots = self._textured(refl, trans)
        return self.add_bsdf(abi.BSDF_DIELECTRIC, [int_ior, ext_ior] + _rgb(refl) + _rgb(trans), slots)

    def roughmetal(self, alpha=0.1, ior=0.37, k=2.82, refl=1.0):
        (refl,), slots = self._textured(refl)
        return self.add_bsdf(abi.BSDF_ROUGHMETAL, [alpha, ior, ior, ior, k, k, k] + _rgb(refl), slots)

    def microfacet(self, alpha=0.1, kd=0.5, ks=0.5, int_ior=1.5, ext_ior=1.0, rd=1.0, rs=1.0):
        (rd, rs), slots = self._textured(rd, rs)
        return self.add_bsdf(abi.BSDF_MICROFACET, [alpha, kd, ks, int_ior, ext_ior] + _rgb(rd) + _rgb(rs), slots)

    def mirror(self, r=0.8):
        (r,), slots = self._textured(r)
        return self.add_bsdf(abi.BSDF_MIRROR, _rgb(r), slots)

    def phong(self, exponent=10.0, rd=0.5, rs=0.2, kd=1.0, ks=1.0):
        """parameter block as Phong::configure() leaves it (src/bsdfs/phong.cpp:74-96), float32 arithmetic"""
        max_d, max_s = max(_rgb(_slot_maximum(rd))), max(_rgb(_slot_maximum(rs)))      # getMaximum().max()
        (rd, rs), slots = self._textured(rd, rs)
        kd, ks, rd, rs = F(kd), F(ks), _rgb(rd), _rgb(rs)
        if kd * max_d + ks * max_s > F(1.0):                 # verifyEnergyConservation
            norm = F(1) / (kd * max_d + ks * max_s)
            kd, ks = kd * norm, ks * norm
        avg_d = (rd[0] + rd[1] + rd[2]) * F(1.0 / 3) * kd    # getAverage().average() * m_kd
        avg_s = (rs[0] + rs[1] + rs[2]) * F(1.0 / 3) * ks
        ssw = avg_s / (avg_d + avg_s)
        dsw = F(1.0) - ssw
        return self.add_bsdf(abi.BSDF_PHONG, [exponent, kd, ks, ssw, dsw] + rd + rs, slots)

    def roughglass(self, alpha=0.1, int_ior=1.5046, ext_ior=1.0, distribution="beckmann", refl=1.0, trans=1.0):
        """src/bsdfs/roughglass.cpp: for `phong` the constructor maps alpha to the exponent 2/alpha^2 - 2 (:130-136)"""
        d = {"beckmann": 0, "phong": 1, "ggx": 2}[distribution]
        if alpha is VERTEX_COLORS or isinstance(alpha, _UvTexture):
            raise ValueError("roughglass: alpha is a float texture, neither vertex colours nor a uv texture can drive it")
        (refl, trans), slots = self._textured(refl, trans)
        a = F(alpha)
        if d == 1:
            a = F(2) / (a * a) - F(2)
        return self.add_bsdf(abi.BSDF_ROUGHGLASS, [d, a, int_ior, ext_ior] + _rgb(refl) + _rgb(trans), slots)

    def difftrans(self, t=0.5):
        (t,), slots = self._textured(t)
        return self.add_bsdf(abi.BSDF_DIFFTRANS, _rgb(t), slots)

    def ward(self, alpha_x=0.1, alpha_y=0.1, rd=0.5, rs=0.2, kd=1.0, ks=1.0, model="balanced", specular_sampling_weight=-1.0,
             verify_energy_conservation=True):
        """parameter block as the constructor and Ward::configure() leave it (src/bsdfs/ward.cpp:54-88, :118-136), float32
        arithmetic; rd / rs: a grey level or an RGB triple"""
        m = {"ward": 0, "ward-duer": 1, "balanced": 2}[model]
        max_d, max_s = max(_rgb(_slot_maximum(rd))), max(_rgb(_slot_maximum(rs)))      # getMaximum().max()
        (rd, rs), slots = self._textured(rd, rs)
        rd = np.broadcast_to(np.asarray(rd, dtype=np.float32), (3,)); rs = np.broadcast_to(np.asarray(rs, dtype=np.float32), (3,))
        kd, ks = F(kd), F(ks)
        if verify_energy_conservation and kd * max_d + ks * max_s > F(1.0):
            norm = F(1) / (kd * max_d + ks * max_s)
            kd, ks = kd * norm, ks * norm
        ssw = F(specular_sampling_weight)
        if ssw == F(-1):
            avg_d = (rd[0] + rd[1] + rd[2]) * F(1.0 / 3) * kd          # Spectrum::average() * m_kd
            avg_s = (rs[0] + rs[1] + rs[2]) * F(1.0 / 3) * ks
            ssw = avg_s / (avg_d + avg_s)
        dsw = F(1.0) - ssw
        return self.add_bsdf(abi.BSDF_WARD, [m, alpha_x, alpha_y, kd, ks, ssw, dsw, rd[0], rd[1], rd[2], rs[0], rs[1], rs[2]], slots)

    def composite(self, weights, children):
        """<bsdf type="composite"> (src/bsdfs/composite.cpp): weights and the indices of blocks added before.  Block:
        [0] n, [1..n] weights, [1+n..2n] child indices as floats (include/mtsgpu.h); the flattener checks it"""
        weights = [float(w) for w in weights]; children = [int(c) for c in children]
        if len(weights) != len(children):
            raise ValueError("BSDF count mismatch: %d bsdfs, but specified %d weights" % (len(children), len(weights)))   # composite.cpp:98-100
        if 1 + 2 * len(weights) > abi.BSDF_NPARAMS:
            raise ValueError("a composite holds at most %d children" % abi.COMPOSITE_MAX)
        return self.add_bsdf(abi.BSDF_COMPOSITE, [len(weights)] + weights + children)

    def bsdf_is_anisotropic(self, b):
        """BSDF::EAnisotropic of block b: a Ward with alphaU != alphaV (ward.cpp:84-85), alone or as a composite's child; the
        twosided adapter passes its child's type on"""
        t, P = self.bsdf_type[b] & 0xFF, self.bsdf_params[b]
        if t == abi.BSDF_WARD:
            return bool(P[1] != P[2])
        if t == abi.BSDF_COMPOSITE:
            n = int(P[0])
            return any(self.bsdf_is_anisotropic(int(P[1 + n + i])) for i in range(n))
        return False

    def twosided(self, bsdf):
        """wrap an existing BSDF block in the `twosided` adapter (src/bsdfs/twosided.cpp)"""
        self.bsdf_type[bsdf] |= abi.BSDF_TWOSIDED
        return bsdf

    def mask(self, bsdf, opacity=0.5):
        """wrap an existing BSDF block in the `mask` adapter (src/bsdfs/mask.cpp): opacity is a grey level, an RGB triple or a
        Checkerboard / GridTexture / BitmapTexture.  The mask is the outermost adapter: call it last, after twosided()"""
        if opacity is VERTEX_COLORS:
            raise ValueError("mask: vertex colours as opacity are not supported")
        if bsdf in self.bsdf_masks:
            raise ValueError("mask: BSDF %d has a mask already, nested masks are not supported" % bsdf)
        if self.bsdf_type[bsdf] & 0xFF == abi.BSDF_COMPOSITE:
            raise ValueError("mask: a mask around a composite is not supported")
        for b, t in enumerate(self.bsdf_type):
            n = int(self.bsdf_params[b][0])
            if t & 0xFF == abi.BSDF_COMPOSITE and bsdf in [int(c) for c in self.bsdf_params[b][1 + n:1 + 2 * n]]:
                raise ValueError("mask: BSDF %d is a child of composite %d, a mask inside a composite is not supported" % (bsdf, b))
        if isinstance(opacity, _UvTexture):
            if not any(opacity is u for u in self.textures):
                self.textures.append(opacity)
        else:
            opacity = np.array(_rgb(opacity), dtype=np.float32)
            if not np.isfinite(opacity).all():
                raise ValueError("mask: the opacity is not finite")
        self.bsdf_masks[int(bsdf)] = opacity
        return bsdf

    def mask_table(self):
        """one (kind, texture index, opacity rgb) per BSDF: what mtsgpu_bsdf_mask holds; a textured mask's three floats are the
        texture's getAverage()"""
        rows = []
        for b in range(len(self.bsdf_type)):
            o = self.bsdf_masks.get(b)
            if o is None:
                rows.append((abi.MASK_NONE, -1, [F(0), F(0), F(0)]))
            elif isinstance(o, _UvTexture):
                rows.append((abi.MASK_TEXTURE, [i for i, u in enumerate(self.textures) if u is o][0], _rgb(o.average())))
            else:
                rows.append((abi.MASK_CONSTANT, -1, _rgb(o)))
        return rows

    def wiscombe(self, g=0.874, depth=1.0, w0=0.99, sigma_t=(16.4967, 6.0957, 4.6547)):
        """<bsdf type="wiscombe"> with the reference's defaults (wiscombe.cpp:44-55): a Lambertian entry whose block is zero and
        is not read, with a snow record; raw = g, depth, w0 rgb, sigmaT rgb (what Wiscombe::serialize writes)"""
        b = self.add_bsdf(abi.BSDF_LAMBERTIAN, [0.0, 0.0, 0.0])
        self.bsdf_snow[b] = (abi.SNOW_WISCOMBE, np.array([F(g), F(depth)] + _rgb(w0) + _rgb(sigma_t), dtype=np.float32))
        return b

    def hanrahan_krueger(self, sigma_a=(0.0014, 0.0025, 0.0142), sigma_s=(0.7, 1.22, 1.9), size_multiplier=1.0, g=0.0, eta_int=1.32,
                         eta_ext=1.0, ss_factor=1.0, dr_factor=1.0, diffuse_reflectance=True):
        """<bsdf type="hanrahankrueger"> with the reference's defaults (hanrahan-krueger.cpp:46-74): as wiscombe(); raw = sigmaA
        rgb, sigmaS rgb (both times the size multiplier, in binary32), g, etaInt, etaExt, ssFactor rgb, drFactor rgb, the flag"""
        m = F(size_multiplier)
        raw = [F(x) * m for x in _rgb(sigma_a)] + [F(x) * m for x in _rgb(sigma_s)] + [F(g), F(eta_int), F(eta_ext)] \
            + _rgb(ss_factor) + _rgb(dr_factor) + [F(1.0 if diffuse_reflectance else 0.0)]
        b = self.add_bsdf(abi.BSDF_LAMBERTIAN, [0.0, 0.0, 0.0])
        self.bsdf_snow[b] = (abi.SNOW_HK, np.array(raw, dtype=np.float32))
        return b

    def snow_table(self, configure=None):
        """one entry per BSDF: what mtsgpu_bsdf_snow holds, None for a BSDF without a snow record.  configure(kind, raw) is the
        reference's configure() -- by default the library's own (snow_configure: mtsgpu_wiscombe_configure, mtsgpu_hk_configure)"""
        if configure is None:
            from . import snow_configure as configure
        return [configure(*self.bsdf_snow[b]) if b in self.bsdf_snow else None for b in range(len(self.bsdf_type))]

    def irawan(self, weave, repeat_u=None, repeat_v=None, kd_multiplier=None, ks_multiplier=None):
        """<bsdf type="irawan">: a Lambertian entry whose block is zero and is not read, with the Weave `weave` (load_weave); the
        four properties of the plugin (irawan.cpp:80-85) override the weave's own when given"""
        over = dict(repeatU=repeat_u, repeatV=repeat_v, kdMultiplier=kd_multiplier, ksMultiplier=ks_multiplier)
        if any(v is not None for v in over.values()):
            weave = weave.replace(**{k: v for k, v in over.items() if v is not None})
        b = self.add_bsdf(abi.BSDF_LAMBERTIAN, [0.0, 0.0, 0.0])
        if not any(weave is w for w in self.weaves):
            self.weaves.append(weave)
        self.bsdf_weave[b] = [i for i, w in enumerate(self.weaves) if w is weave][0]
        return b

    def weave_table(self):
        """one weave index per BSDF, -1 for a BSDF without one (what mtsgpu_set_cloth_bsdfs takes as bsdf_weave)"""
        return np.asarray([self.bsdf_weave.get(b, -1) for b in range(len(self.bsdf_type))], dtype=np.int32)

    def point_light(self, position, intensity):
        l = self.add_lum(abi.LUM_POINT, [intensity] * 3 if np.isscalar(intensity) else intensity)
        self.lum_params[l][3:6] = np.asarray(position, dtype=np.float32)
        return l

    def directional_light(self, direction, intensity):
        l = self.add_lum(abi.LUM_DIRECTIONAL, [intensity] * 3 if np.isscalar(intensity) else intensity)
        d = np.asarray(direction, dtype=np.float32)
        self.lum_params[l][3:6] = d / np.sqrt((d * d).sum(), dtype=np.float32)
        return l

    def spot_light(self, position, target, intensity, cutoff_deg=20.0, beam_deg=None, texture=None, bilinear=False):
        """SpotLuminaire with toWorld = lookAt(position, target, up) (src/luminaires/spot.cpp:33-62).  texture: its projection
        texture (:95-101), a Checkerboard, GridTexture or BitmapTexture object; bilinear: a BitmapTexture is looked up as
        filterType trilinear / ewa are without uv partials, MIPMap::triangle(0, ., .), instead of the nearest texel (none)"""
        l = self.add_lum(abi.LUM_SPOT, [intensity] * 3 if np.isscalar(intensity) else intensity)
        P = self.lum_params[l]
        pos, tgt = np.asarray(position, dtype=np.float32), np.asarray(target, dtype=np.float32)
        d = tgt - pos; d = d / np.sqrt((d * d).sum(), dtype=np.float32)
        up = np.array([0, 0, 1], dtype=np.float32) if abs(d[2]) < 0.9 else np.array([1, 0, 0], dtype=np.float32)
        right = np.cross(d, up).astype(np.float32); right /= np.sqrt((right * right).sum(), dtype=np.float32)
        new_up = np.cross(right, d).astype(np.float32)
        P[3:6] = pos
        beam = cutoff_deg * 0.75 if beam_deg is None else beam_deg
        P[8] = F(cutoff_deg) * (F(np.pi) / F(180.0))         # degToRad
        P[19] = F(beam) * (F(np.pi) / F(180.0))
        P[10:13] = right; P[13:16] = new_up; P[16:19] = d    # world -> luminaire rotation (rows)
        if texture is not None:
            if not isinstance(texture, _UvTexture):
                raise TypeError("spot_light: texture is a Checkerboard, GridTexture or BitmapTexture")
            if not hasattr(self, "spot_textures"):
                self.spot_textures = {}
            self.spot_textures[l] = (texture, bool(bilinear))
        return l

    def spot_texture_table(self):
        """(textures, texture_bilinear [n_textures] uint32, lum_texture [n_lums] int32) of the spot luminaires with a projection
        texture: what mtsgpu_set_spot_textures takes, one texture entry per textured luminaire"""
        st = getattr(self, "spot_textures", {})
        textures, flags = [], []
        lum = np.full(len(self.lum_type), -1, dtype=np.int32)
        for l in sorted(st):
            lum[l] = len(textures)
            textures.append(st[l][0]); flags.append(1 if st[l][1] else 0)
        return textures, np.asarray(flags, dtype=np.uint32), lum

    def collimated_beam(self, position, target, intensity, radius=0.01):
        """<luminaire type="collimated"> with toWorld = lookAt(position, target) (src/luminaires/collimated.cpp)"""
        l = self.add_lum(abi.LUM_COLLIMATED, [intensity] * 3 if np.isscalar(intensity) else intensity)
        P = self.lum_params[l]
        pos, tgt = np.asarray(position, dtype=np.float32), np.asarray(target, dtype=np.float32)
        d = tgt - pos; d = d / np.sqrt((d * d).sum(), dtype=np.float32)
        up = np.array([0, 0, 1], dtype=np.float32) if abs(d[2]) < 0.9 else np.array([1, 0, 0], dtype=np.float32)
        right = np.cross(d, up).astype(np.float32); right /= np.sqrt((right * right).sum(), dtype=np.float32)
        new_up = np.cross(right, d).astype(np.float32)
        R = np.stack([right, new_up, d], axis=1).astype(np.float32)          # luminaire -> world (columns)
        P[3] = radius
        L2W = np.concatenate([R, pos.reshape(3, 1)], axis=1).astype(np.float32)
        Rt = R.T.astype(np.float32)
        W2L = np.concatenate([Rt, (-(Rt @ pos)).reshape(3, 1)], axis=1).astype(np.float32)
        P[4:16] = W2L.ravel(); P[16:28] = L2W.ravel()
        return l

    def envmap(self, bitmap, intensity_scale=1.0, to_world=None):
        """<luminaire type="envmap"> (src/luminaires/envmap.cpp): lat-long bitmap [H][W][3], optional rotation"""
        l = self.add_lum(abi.LUM_ENVMAP, [intensity_scale, 0, 0])
        R = np.eye(3, dtype=np.float32) if to_world is None else np.asarray(to_world, dtype=np.float32).reshape(3, 3)
        self.lum_params[l][16:25] = R.ravel()
        self.env_bitmap = np.ascontiguousarray(bitmap, dtype=np.float32)
        assert self.env_bitmap.ndim == 3 and self.env_bitmap.shape[2] == 3
        return l

    def sky(self, sun_direction=None, latitude=None, longitude=None, standard_meridian=None, julian_day=None, time_of_day=None,
            turbidity=2.0, sky_scale=1.0, a=1.0, b=1.0, c=1.0, d=1.0, e=1.0, clip_below_horizon=True, to_world=None):
        """<luminaire type="sky"> as its constructor leaves it (src/luminaires/sky.cpp:47-103), float32 arithmetic: the sun
        is placed EITHER by a direction (+x south, +y east, +z up) OR by latitude, longitude, standardMeridian, julianDay and
        timeOfDay, all five; with neither, the defaults of the reference apply.  to_world: 3x3 rotation (row major).  The
        block holds world->luminaire = inverse(rotate(x, -90 deg) * toWorld), thetaS and phiS; the flattener adds the
        bounding sphere."""
        loc = [latitude, longitude, standard_meridian, julian_day, time_of_day]
        has_dir, has_some, has_all = sun_direction is not None, any(v is not None for v in loc), all(v is not None for v in loc)
        if not (has_dir or has_some):
            has_some = has_all = True
        elif has_dir and has_some:
            raise ValueError("Please decide for either positioning the sun by a direction vector or by some location and time information.")
        elif has_some and not has_all:
            raise ValueError("Please give all required parameters for specifing the sun's position by location and time information. "
                             "At least one is missing.")
        if has_dir:
            theta_s, phi_s = sky_sun_from_direction(sun_direction)
        else:
            dflt = [51.050891, 13.694458, 0, 200, 22.00]
            theta_s, phi_s = sky_sun_from_location(*[dv if v is None else v for v, dv in zip(loc, dflt)])
        # Transform::rotate(Vector(1, 0, 0), -90) (transform.cpp:72-98) * toWorld, and its inverse (a rotation: the transpose)
        ang = F(-90.0) * (F(np.pi) / F(180.0))                 # degToRad
        sn, cs = F(np.sin(ang)), F(np.cos(ang))
        rot = np.array([[1, 0, 0], [0, cs, -sn], [0, sn, cs]], dtype=np.float32)
        tw = np.eye(3, dtype=np.float32) if to_world is None else np.asarray(to_world, dtype=np.float32).reshape(3, 3)
        l2w = (rot.astype(np.float64) @ tw.astype(np.float64)).astype(np.float32)
        w2l = np.linalg.inv(l2w.astype(np.float64)).astype(np.float32)
        l = self.add_lum(abi.LUM_SKY, [sky_scale, turbidity, 1.0 if clip_below_horizon else 0.0])
        P = self.lum_params[l]
        P[7:16] = w2l.ravel()
        P[16], P[17] = theta_s, phi_s
        P[18:23] = np.asarray([a, b, c, d, e], dtype=np.float32)
        return l

    def add_lum(self, ltype, intensity):
        p = np.zeros(abi.LUM_NPARAMS, dtype=np.float32)
        p[:3] = np.asarray(intensity, dtype=np.float32)
        self.lum_type.append(int(ltype))
        self.lum_params.append(p)
        return len(self.lum_type) - 1

    def add_mesh(self, *a, **k):
        self.meshes.append(MeshDesc(*a, **k))
        return self.meshes[-1]

    def add_sphere(self, *a, **k):
        self.meshes.append(SphereDesc(*a, **k))
        return self.meshes[-1]

    def add_cylinder(self, p1=None, p2=None, radius=None, to_world=None, bsdf=-1, lum=-1, name="cylinder"):
        """add_cylinder(p1, p2, radius, bsdf=...) or add_cylinder(to_world=..., bsdf=...)"""
        self.meshes.append(CylinderDesc(p1, p2, radius, to_world, bsdf, lum, name))
        return self.meshes[-1]

    @property
    def n_tris(self):
        return sum(m.triangles.shape[0] for m in self.meshes)

    # --- ctypes view --------------------------------------------------------
    def to_ctypes(self):
        """-> (mtsgpu_scene_desc, keepalive list)"""
        keep = []
        meshes = (abi.Mesh * len(self.meshes))()
        for i, m in enumerate(self.meshes):
            keep += [m.positions, m.triangles, m.normals]
            meshes[i].n_verts = m.positions.shape[0]
            meshes[i].n_tris = m.triangles.shape[0]
            meshes[i].positions = abi.ptr(m.positions, abi.f32p)
            meshes[i].normals = abi.ptr(m.normals, abi.f32p)
            meshes[i].triangles = abi.ptr(m.triangles, abi.u32p)
            meshes[i].face_normals = 1 if m.face_normals else 0
            meshes[i].bsdf = m.bsdf
            meshes[i].lum = m.lum
            meshes[i].shape_type = m.shape_type
            if m.sphere is not None:
                meshes[i].sphere_center = (C.c_float * 3)(*m.sphere[0])
                meshes[i].sphere_radius = m.sphere[1]
                meshes[i].sphere_inverted = 1 if m.sphere[2] else 0
        bt = np.asarray(self.bsdf_type, dtype=np.uint32)
        bp = np.ascontiguousarray(np.stack(self.bsdf_params) if self.bsdf_params else np.zeros((0, abi.BSDF_NPARAMS)), dtype=np.float32)
        lt = np.asarray(self.lum_type, dtype=np.uint32)
        lp = np.ascontiguousarray(np.stack(self.lum_params) if self.lum_params else np.zeros((0, abi.LUM_NPARAMS)), dtype=np.float32)
        d = abi.SceneDesc()
        d.n_meshes = len(self.meshes)
        d.meshes = C.cast(meshes, C.POINTER(abi.Mesh))
        d.n_bsdfs = len(bt)
        d.bsdf_type = abi.ptr(bt, abi.u32p)
        d.bsdf_params = abi.ptr(bp, abi.f32p)
        d.n_lums = len(lt)
        d.lum_type = abi.ptr(lt, abi.u32p)
        d.lum_params = abi.ptr(lp, abi.f32p)
        d.camera_pos = (C.c_float * 3)(*[float(v) for v in self.camera["origin"]])
        d.has_camera = 1
        if self.env_bitmap is not None:
            d.env_width, d.env_height = self.env_bitmap.shape[1], self.env_bitmap.shape[0]
            d.env_bitmap = abi.ptr(self.env_bitmap, abi.f32p)
            keep.append(self.env_bitmap)
        keep += [meshes, bt, bp, lt, lp]
        return d, keep


# ---------------------------------------------------------------------------
# the sun of the sky luminaire
# ---------------------------------------------------------------------------
def sky_sun_from_direction(sun_direction):
    """SkyLuminaire::configureSunPosition(const Vector &) (sky.cpp:214-219): toSphericalCoordinates of the normalised
    direction (util.cpp:618-626) -> (thetaS, phiS) as float32"""
    v = np.asarray(sun_direction, dtype=np.float32)
    v = v * (F(1) / np.sqrt((v * v).sum(dtype=np.float32), dtype=np.float32))
    theta = F(np.arccos(np.float64(np.clip(v[2], -1, 1))))
    phi = F(np.arctan2(np.float64(v[1]), np.float64(v[0])))
    if phi < 0:
        phi = phi + F(2) * F(np.pi)                          # M_PI is a float literal in the single-precision build (constants.h:45-46)
    return theta, phi


def sky_sun_from_location(lat, lon, std_mrd, jul_day, time_of_day):
    """SkyLuminaire::configureSunPosition(lat, lon, int stdMrd, int julDay, timeOfDay) (sky.cpp:186-208, IES Lighting
    Handbook p. 361): standardMeridian and julianDay are truncated to int by the call; M_PI is a float, double literals
    promote their expression to double, every const Float rounds to float32"""
    D = np.float64
    lat, lon, time_of_day = F(lat), F(lon), F(time_of_day)
    std_mrd, jul_day = int(F(std_mrd)), int(F(jul_day))
    pi = F(np.pi)
    solar_time = F(D(time_of_day)
                   + (0.170 * np.sin(4.0 * D(pi) * (jul_day - 80.0) / 373.0) - 0.129 * np.sin(2.0 * D(pi) * (jul_day - 8.0) / 355.0))
                   + D(F(std_mrd) - lon) / 15.0)
    decl = F(0.4093 * D(np.sin(F(2) * pi * F(jul_day - 81) / F(368))))
    rlat = lat * (pi / F(180.0))                             # degToRad
    hour = D(pi * solar_time) / 12.0
    altitude = F(np.arcsin(D(np.sin(rlat) * np.sin(decl)) - D(np.cos(rlat) * np.cos(decl)) * np.cos(hour)))
    opp = F(D(-np.cos(decl)) * np.sin(hour))
    adj = F(-(D(np.cos(rlat) * np.sin(decl)) + D(np.sin(rlat) * np.cos(decl)) * np.cos(hour)))
    azimuth = F(np.arctan2(opp, adj))
    return F(D(pi) / 2.0 - D(altitude)), F(-azimuth)


# ---------------------------------------------------------------------------
# geometry helpers
# ---------------------------------------------------------------------------
def _quad(p0, e1, e2, want_normal):
    """two triangles covering p0 + s*e1 + t*e2, wound so that cross(p1-p0, p2-p0) points along want_normal"""
    p0, e1, e2 = (np.asarray(v, dtype=np.float32) for v in (p0, e1, e2))
    if np.dot(np.cross(e1, e2), np.asarray(want_normal, dtype=np.float32)) < 0:
        e1, e2 = e2, e1
    pos = np.stack([p0, p0 + e1, p0 + e1 + e2, p0 + e2]).astype(np.float32)
    tri = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32)
    return pos, tri


def hash32(a, b, c, seed=1):
    """fixed integer mixer (uint32 arithmetic), vectorised"""
    with np.errstate(over="ignore"):
        h = (np.asarray(a, dtype=np.uint32) * np.uint32(0x9E3779B1)
             ^ np.asarray(b, dtype=np.uint32) * np.uint32(0x85EBCA77)
             ^ np.asarray(c, dtype=np.uint32) * np.uint32(0xC2B2AE3D)
             ^ np.uint32(seed) * np.uint32(0x27D4EB2F))
        h ^= h >> np.uint32(15)
        h *= np.uint32(0x2C1B3C6D)
        h ^= h >> np.uint32(12)
        h *= np.uint32(0x297A2D39)
        h ^= h >> np.uint32(15)
    return h


def _grid_face(face_id, p0, e1, e2, normal, n, amp):
    """n x n grid of cells x 2 triangles with unshared vertices; interior grid points are
    displaced along `normal` by amp*(hash/2^32 - 0.5); border points stay put (watertight box)."""
    p0, e1, e2, normal = (np.asarray(v, dtype=np.float32) for v in (p0, e1, e2, normal))
    if np.dot(np.cross(e1, e2), normal) < 0:
        e1, e2 = e2, e1
    ii, jj = np.meshgrid(np.arange(n + 1, dtype=np.uint32), np.arange(n + 1, dtype=np.uint32), indexing="ij")
    s = ii.astype(np.float32) / F(n)
    t = jj.astype(np.float32) / F(n)
    disp = (hash32(np.uint32(face_id), ii, jj).astype(np.float32) / F(4294967296.0) - F(0.5)) * F(amp)
    border = (ii == 0) | (ii == n) | (jj == 0) | (jj == n)
    disp = np.where(border, F(0), disp).astype(np.float32)
    grid = (p0[None, None, :] + s[..., None] * e1[None, None, :] + t[..., None] * e2[None, None, :]
            + disp[..., None] * normal[None, None, :]).astype(np.float32)
    a = grid[:-1, :-1]; b = grid[1:, :-1]; c = grid[1:, 1:]; d = grid[:-1, 1:]
    # two triangles per cell: (a, b, c), (a, c, d); 6 unshared vertices per cell
    pos = np.stack([a, b, c, a, c, d], axis=2).reshape(-1, 3).astype(np.float32)
    tri = np.arange(pos.shape[0], dtype=np.uint32).reshape(-1, 3)
    return pos, tri


def icosphere(subdiv, radius, centre):
    """icosahedron subdivided `subdiv` times, shared vertices, outward winding"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2],
                  [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5],
                  [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], dtype=np.int64)
    for _ in range(subdiv):
        edges = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0)
        es = np.sort(edges, axis=1)
        uniq, inv = np.unique(es, axis=0, return_inverse=True)
        mid = v[uniq[:, 0]] + v[uniq[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        base = v.shape[0]
        v = np.concatenate([v, mid], axis=0)
        nf = f.shape[0]
        inv = inv.reshape(-1)
        m01, m12, m20 = base + inv[:nf], base + inv[nf:2 * nf], base + inv[2 * nf:]
        f = np.concatenate([
            np.stack([f[:, 0], m01, m20], axis=1), np.stack([f[:, 1], m12, m01], axis=1),
            np.stack([f[:, 2], m20, m12], axis=1), np.stack([m01, m12, m20], axis=1)], axis=0)
    pos = (v * radius + np.asarray(centre, dtype=np.float64)[None, :]).astype(np.float32)
    # make sure the winding is outward (cross(p1-p0, p2-p0) . (centroid - centre) > 0)
    p = v[f]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    flip = np.einsum("ij,ij->i", n, p.mean(axis=1)) < 0
    f[flip] = f[flip][:, [0, 2, 1]]
    return pos, f.astype(np.uint32)


# ---------------------------------------------------------------------------
# configurations
# ---------------------------------------------------------------------------
def _box_faces():
    # (name, p0, e1, e2, inward normal)
    return [
        ("floor",   (-1, 0, -1), (2, 0, 0), (0, 0, 2), (0, 1, 0)),
        ("ceiling", (-1, 2, -1), (2, 0, 0), (0, 0, 2), (0, -1, 0)),
        ("back",    (-1, 0, -1), (2, 0, 0), (0, 2, 0), (0, 0, 1)),
        ("left",    (-1, 0, -1), (0, 0, 2), (0, 2, 0), (1, 0, 0)),
        ("right",   (1, 0, -1),  (0, 0, 2), (0, 2, 0), (-1, 0, 0)),
    ]


def _add_light(sd, intensity=15.0):
    black = sd.lambertian(0.0)
    lum = sd.add_lum(abi.LUM_AREA, [intensity] * 3)
    pos, tri = _quad((-0.25, 1.99, -0.25), (0.5, 0, 0), (0, 0, 0.5), (0, -1, 0))
    sd.add_mesh(pos, tri, bsdf=black, lum=lum, face_normals=True, name="light")


def cornell_c1():
    """C1/C2: 6 quads / 12 triangles, lambertian walls, one area luminaire"""
    sd = SceneDescription("cornell_c1")
    white = sd.lambertian(0.73)
    red = sd.lambertian(0.63, 0.065, 0.05)
    green = sd.lambertian(0.14, 0.45, 0.091)
    for name, p0, e1, e2, nrm in _box_faces():
        pos, tri = _quad(p0, e1, e2, nrm)
        sd.add_mesh(pos, tri, bsdf={"left": red, "right": green}.get(name, white), face_normals=True, name=name)
    _add_light(sd)
    sd.max_depth = 4
    return sd


def cornell_c3(grid=320, sphere_subdiv=5):
    """C3/C4: one displaced walls TriMesh (5 faces x grid^2 x 2 tris; 1 024 000 at grid=320),
    a dielectric icosphere and the light quad"""
    sd = SceneDescription("cornell_c3_g%d" % grid)
    white = sd.lambertian(0.73)
    glass = sd.dielectric(1.5046, 1.0)
    ps, ts, base = [], [], 0
    for fid, (name, p0, e1, e2, nrm) in enumerate(_box_faces()):
        pos, tri = _grid_face(fid, p0, e1, e2, nrm, grid, 0.01)
        ps.append(pos); ts.append(tri + np.uint32(base)); base += pos.shape[0]
    sd.add_mesh(np.concatenate(ps), np.concatenate(ts), bsdf=white, face_normals=True, name="walls")
    pos, tri = icosphere(sphere_subdiv, 0.4, (0.3, 0.4, 0.2))
    sd.add_mesh(pos, tri, bsdf=glass, face_normals=False, name="glass")
    _add_light(sd)
    sd.max_depth = 16
    return sd


def cornell_c5(sphere_subdiv=4):
    """C5: C1 box + four icospheres (lambertian, roughmetal, dielectric, microfacet) + constant env"""
    sd = cornell_c1()
    sd.name = "cornell_c5"
    mats = [sd.lambertian(0.5), sd.roughmetal(), sd.dielectric(), sd.microfacet()]
    centres = [(-0.5, 0.3, -0.4), (0.5, 0.3, -0.4), (-0.5, 0.3, 0.45), (0.5, 0.3, 0.45)]
    for m, c in zip(mats, centres):
        pos, tri = icosphere(sphere_subdiv, 0.3, c)
        sd.add_mesh(pos, tri, bsdf=m, face_normals=False, name="sphere")
    sd.add_lum(abi.LUM_CONSTANT, [1.0, 1.0, 1.0])
    sd.max_depth = 32
    return sd


def next_rows(sphere_subdiv=2):
    """mirror / phong / twosided BSDFs, point / spot / directional luminaires, thin lens"""
    sd = SceneDescription("next_rows")
    white = sd.twosided(sd.lambertian(0.73))
    red = sd.twosided(sd.lambertian(0.63, 0.065, 0.05))
    green = sd.lambertian(0.14, 0.45, 0.091)
    for name, p0, e1, e2, nrm in _box_faces():
        pos, tri = _quad(p0, e1, e2, nrm)
        if name == "back":
            tri = tri[:, [0, 2, 1]]                 # wound the wrong way round: only a twosided BSDF shades it
        sd.add_mesh(pos, tri, bsdf={"left": red, "right": green}.get(name, white), face_normals=True, name=name)
    _add_light(sd, intensity=6.0)
    mats = [sd.mirror(0.8), sd.phong(20.0, 0.4, 0.3), sd.twosided(sd.roughmetal(0.2)), sd.phong(5.0, 0.9, 0.6)]
    centres = [(-0.5, 0.3, -0.4), (0.5, 0.3, -0.4), (-0.5, 0.3, 0.45), (0.5, 0.3, 0.45)]
    for m, c in zip(mats, centres):
        pos, tri = icosphere(sphere_subdiv, 0.3, c)
        sd.add_mesh(pos, tri, bsdf=m, face_normals=False, name="sphere")
    # a diffusely transmitting sheet in front of the back wall and a collimated beam onto the floor
    pos, tri = _quad((-0.6, 0.9, -0.7), (1.2, 0, 0), (0, 0.7, 0), (0, 0, 1))
    sd.add_mesh(pos, tri, bsdf=sd.difftrans(0.6), face_normals=True, name="sheet")
    sd.collimated_beam((0.1, 1.9, 0.1), (0.1, 0.0, 0.1), 6.0, radius=0.15)
    sd.point_light((0.0, 1.2, 0.6), 0.6)
    sd.spot_light((-0.8, 1.8, 0.8), (0.4, 0.0, -0.3), 25.0, cutoff_deg=25.0)
    sd.directional_light((0.3, -1.0, -0.4), 0.4)
    sd.camera["aperture"] = 0.04
    sd.camera["focus"] = 3.3
    sd.max_depth = 8
    return sd


def spheres():
    """analytic `sphere` shapes (glass, mirror, diffuse, one inverted) and a sphere-shaped
    area luminaire (Sphere::sampleSolidAngle) next to a mesh luminaire, inside the Cornell box"""
    sd = SceneDescription("spheres")
    white = sd.lambertian(0.73)
    red = sd.lambertian(0.63, 0.065, 0.05)
    green = sd.lambertian(0.14, 0.45, 0.091)
    for name, p0, e1, e2, nrm in _box_faces():
        pos, tri = _quad(p0, e1, e2, nrm)
        sd.add_mesh(pos, tri, bsdf={"left": red, "right": green}.get(name, white), face_normals=True, name=name)
    _add_light(sd, intensity=4.0)
    sd.add_sphere((-0.45, 0.35, -0.3), 0.35, bsdf=sd.dielectric())
    sd.add_sphere((0.5, 0.3, 0.3), 0.3, bsdf=sd.mirror(0.9))
    sd.add_sphere((0.0, 0.2, 0.55), 0.2, bsdf=sd.lambertian(0.3, 0.4, 0.8))
    sd.add_sphere((0.45, 1.3, -0.4), 0.25, bsdf=sd.twosided(sd.phong(30.0, 0.3, 0.5)), inverted=True)
    sd.add_sphere((-0.75, 0.15, 0.6), 0.15, bsdf=sd.roughglass(0.15, 1.5, 1.0, "beckmann"))
    sd.add_sphere((-0.25, 0.12, 0.8), 0.12, bsdf=sd.roughglass(0.4, 1.5, 1.0, "ggx"))
    sd.add_sphere((0.75, 0.12, 0.8), 0.12, bsdf=sd.roughglass(0.3, 1.33, 1.0, "phong", trans=0.9))
    lum = sd.add_lum(abi.LUM_AREA, [9.0, 7.0, 4.0])
    sd.add_sphere((-0.55, 1.45, 0.35), 0.12, bsdf=sd.lambertian(0.0), lum=lum)
    sd.max_depth = 8
    return sd


def env_bitmap(width=96, height=40, seed=5):
    """a synthetic HDR lat-long image: sky gradient, a small hot sun, ground colour, hash noise (not a power of two,
    so MIPMap's Lanczos up-sampling runs)"""
    y, x = np.mgrid[0:height, 0:width].astype(np.float32)
    v = (y + F(0.5)) / F(height)
    img = np.zeros((height, width, 3), dtype=np.float32)
    sky = (F(1) - v)[..., None] * np.array([0.5, 0.7, 1.2], dtype=np.float32) + F(0.15)
    ground = np.array([0.25, 0.2, 0.12], dtype=np.float32)
    img[:] = np.where((v < F(0.55))[..., None], sky, ground)
    sx, sy = int(width * 0.3), int(height * 0.22)
    img[sy:sy + 2, sx:sx + 3] = np.array([60.0, 55.0, 40.0], dtype=np.float32)
    h = (x.astype(np.uint32) * np.uint32(73856093) ^ y.astype(np.uint32) * np.uint32(19349663) ^ np.uint32(seed * 83492791)) & np.uint32(0xFFFF)
    img *= (F(0.9) + F(0.2) * h.astype(np.float32) / F(65535.0))[..., None]
    return img


def envlit():
    """an `envmap` luminaire (rotated) lights glossy / diffuse / glass objects on a ground plane"""
    sd = SceneDescription("envlit")
    grey = sd.lambertian(0.5)
    pos, tri = _quad((-3.0, 0.0, -3.0), (6.0, 0, 0), (0, 0, 6.0), (0, 1, 0))
    sd.add_mesh(pos, tri, bsdf=grey, face_normals=True, name="ground")
    pos, tri = icosphere(2, 0.4, (-0.7, 0.4, 0.0))
    sd.add_mesh(pos, tri, bsdf=sd.roughmetal(0.15), face_normals=False, name="metal")
    sd.add_sphere((0.3, 0.45, -0.2), 0.45, bsdf=sd.dielectric())
    sd.add_sphere((1.1, 0.3, 0.5), 0.3, bsdf=sd.phong(40.0, 0.5, 0.3))
    c, s_ = F(np.cos(0.7)), F(np.sin(0.7))
    sd.envmap(env_bitmap(), 0.4, to_world=[[c, 0, s_], [0, 1, 0], [-s_, 0, c]])
    sd.camera = dict(origin=(0.2, 1.3, 3.6), target=(0.1, 0.4, 0.0), up=(0.0, 1.0, 0.0), fov=40.0)
    sd.max_depth = 6
    return sd


def matpreview(serialized_path, loader, material="roughglass"):
    """The reference's material-preview scene (data/blender/mitsuba/matpreview/matpreview.xml): the three shapes of
    matpreview.serialized (interior, exterior, ground plane) with the toWorld transforms, camera and envmap rotation
    of the XML; the EXR of the original is replaced by the synthetic lat-long bitmap (no OpenEXR here) and the
    checkerboard of the plane by its mean reflectance.  `loader(path, index)` -> MeshDesc (the product's
    mtsgpu_load_serialized in tests)."""
    sd = SceneDescription("matpreview")
    diff = sd.lambertian(0.18)
    plane = sd.lambertian(0.3)
    mat = {"roughglass": lambda: sd.roughglass(0.1, 1.5046, 1.0, "beckmann"), "roughmetal": lambda: sd.roughmetal(0.1),
           "phong": lambda: sd.phong(30.0, 0.2, 0.7), "dielectric": lambda: sd.dielectric()}[material]()
    inner = loader(serialized_path, 0)
    inner.positions = (inner.positions + np.array([0, 0, 0.0252155], dtype=np.float32)).astype(np.float32)
    inner.bsdf = diff
    outer = loader(serialized_path, 1)
    outer.bsdf = mat
    ground = loader(serialized_path, 2)
    ground.positions = (ground.positions * F(20.0) + np.array([-10, 10, 0], dtype=np.float32)).astype(np.float32)
    ground.bsdf = plane
    sd.meshes += [inner, outer, ground]
    sd.envmap(env_bitmap(), 1.0, to_world=[[-0.224951, -0.000001, -0.974370], [-0.974370, 0.0, 0.224951], [0.0, 1.0, -0.000001]])
    o = np.array([3.69558, -3.46243, 3.25463], dtype=np.float32)
    fwd = np.array([-0.654862, 0.610666, -0.445245], dtype=np.float32)
    sd.camera = dict(origin=tuple(o), target=tuple(o + fwd), up=(-0.31737, 0.312469, 0.895343), fov=28.8415)
    sd.max_depth = 8
    return sd


def bunny(serialized_path, loader, material="roughglass"):
    """The Stanford bunny of the reference's kd-tree test (data/tests/bunny.ply) read back from a `.serialized`
    container through `loader(path, index)`, on a ground plane under the synthetic environment map"""
    sd = SceneDescription("bunny")
    mat = {"roughglass": lambda: sd.roughglass(0.1, 1.5046, 1.0, "beckmann"), "roughmetal": lambda: sd.roughmetal(0.1),
           "lambertian": lambda: sd.lambertian(0.6)}[material]()
    mesh = loader(serialized_path, 0)
    mesh.bsdf = mat
    mesh.face_normals = False
    ground = loader(serialized_path, 1)
    ground.bsdf = sd.lambertian(0.4)
    sd.meshes += [mesh, ground]
    sd.envmap(env_bitmap(), 0.6)
    sd.camera = dict(origin=(-0.05, 0.2, 0.35), target=(-0.02, 0.1, 0.0), up=(0.0, 1.0, 0.0), fov=35.0)
    sd.max_depth = 8
    return sd


def fuzz(seed, n_meshes=14):
    """Random triangle soups, spheres, materials and luminaires inside the Cornell box: shared-vertex meshes with
    smooth normals, degenerate and duplicated triangles, axis-aligned slabs, every BSDF type with random parameters,
    area / point / spot / constant luminaires.  Meant for parity runs (tests/test_gpu_parity.py::test_fuzz_scenes)."""
    rng = np.random.RandomState(seed)
    sd = SceneDescription("fuzz_%d" % seed)
    u = lambda lo, hi, n=None: rng.uniform(lo, hi, n)
    mats = [sd.lambertian(*u(0.1, 0.9, 3)), sd.dielectric(u(1.2, 1.8), 1.0), sd.roughmetal(u(0.05, 0.4)),
            sd.microfacet(u(0.05, 0.4), u(0.2, 0.8), u(0.2, 0.8)), sd.mirror(u(0.5, 0.95)), sd.phong(u(5, 60), u(0.2, 0.6), u(0.1, 0.4)),
            sd.roughglass(u(0.05, 0.3), distribution=["beckmann", "phong", "ggx"][rng.randint(3)]), sd.difftrans(u(0.2, 0.8))]
    mats += [sd.twosided(mats[0]), sd.twosided(mats[3]), sd.twosided(mats[5])]
    white = sd.lambertian(0.73)
    for name, p0, e1, e2, nrm in _box_faces():
        pos, tri = _quad(p0, e1, e2, nrm)
        sd.add_mesh(pos, tri, bsdf=white if rng.rand() < 0.6 else mats[rng.randint(len(mats))], face_normals=True, name=name)
    for m in range(n_meshes):
        kind = rng.randint(5)
        c = np.array([u(-0.8, 0.8), u(0.2, 1.7), u(-0.8, 0.8)])
        bs = mats[rng.randint(len(mats))]
        if kind == 0:                                    # random soup, unshared vertices, some degenerate triangles
            nt = rng.randint(4, 60)
            pos = (c + u(-0.25, 0.25, (nt * 3, 3))).astype(np.float32)
            tri = np.arange(nt * 3, dtype=np.uint32).reshape(nt, 3)
            pos[3 * (nt // 2) + 1] = pos[3 * (nt // 2)]  # two equal vertices
            pos[3 * (nt // 3) + 2] = pos[3 * (nt // 3)] * 0.5 + pos[3 * (nt // 3) + 1] * 0.5      # collinear
            sd.add_mesh(pos, tri, bsdf=bs, face_normals=bool(rng.randint(2)), name="soup%d" % m)
        elif kind == 1:                                  # icosphere with smooth normals
            pos, tri = icosphere(rng.randint(0, 3), u(0.08, 0.3), tuple(c))
            sd.add_mesh(pos, tri, bsdf=bs, face_normals=False, name="ico%d" % m)
        elif kind == 2:                                  # axis-aligned slab: coplanar, duplicated triangles
            pos, tri = _quad(tuple(c), (u(0.1, 0.5), 0, 0), (0, 0, u(0.1, 0.5)), (0, 1, 0))
            tri = np.concatenate([tri, tri])             # every triangle twice
            sd.add_mesh(pos, tri, bsdf=bs, face_normals=True, name="slab%d" % m)
        elif kind == 3:                                  # analytic sphere
            sd.add_sphere(tuple(c), u(0.05, 0.3), bsdf=bs)
        else:                                            # wavy grid with shared vertices (smooth normals)
            n = rng.randint(3, 12)
            gx, gz = np.meshgrid(np.linspace(-0.3, 0.3, n), np.linspace(-0.3, 0.3, n), indexing="ij")
            gy = 0.05 * np.sin(7 * gx + seed) * np.cos(5 * gz)
            pos = (c + np.stack([gx, gy, gz], axis=-1).reshape(-1, 3)).astype(np.float32)
            idx = np.arange(n * n).reshape(n, n)
            a, b, cc, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
            tri = np.concatenate([np.stack([a, b, cc], 1), np.stack([a, cc, d], 1)]).astype(np.uint32)
            sd.add_mesh(pos, tri, bsdf=bs, face_normals=False, name="grid%d" % m)
    _add_light(sd, intensity=float(u(5, 20)))
    extra = rng.randint(4)
    if extra == 0: sd.point_light((u(-0.5, 0.5), u(0.5, 1.5), u(-0.5, 0.5)), (2.0, 2.0, 1.5))
    elif extra == 1: sd.spot_light((0.0, 1.8, 0.5), (u(-0.5, 0.5), 0.0, u(-0.5, 0.5)), (8.0, 8.0, 8.0), cutoff_deg=float(u(15, 40)))
    elif extra == 2: sd.add_lum(abi.LUM_CONSTANT, [0.3, 0.35, 0.5])
    else:                                                # a second area luminaire: an emitting sphere
        lum = sd.add_lum(abi.LUM_AREA, [6.0, 5.0, 4.0])
        sd.add_sphere((u(-0.6, 0.6), u(1.2, 1.7), u(-0.6, 0.6)), 0.08, bsdf=sd.lambertian(0.0), lum=lum)
    sd.max_depth = int(rng.randint(3, 12))
    sd.rr_depth = int(rng.randint(2, 6))
    return sd


def vcol_grid(cells=4, seed=7, material="lambertian", colors="random"):
    """A planar grid of cells x cells x 2 triangles with shared vertices in the plane y = 0 (normal +y) whose (cells + 1)^2
    vertices carry random colours, under one point light, seen straight down by an orthographic camera: every camera ray
    hits the grid at the point below its raster position, so its.color has a closed form.  material: "lambertian"
    (reflectance = vertex colours), "white" (constant reflectance 1), "black", "phong" (specularReflectance = vertex colours,
    slot 1, over a black diffuse part: the radiance stays a multiple of the colour) or "phong_white" (the same with constant
    specularReflectance 1); colors: "random", "zero" or None (a mesh without colours)"""
    sd = SceneDescription("vcol_grid_%d_%s" % (cells, material))
    rng = np.random.RandomState(seed)
    n = cells + 1
    g = np.linspace(-1.0, 1.0, n).astype(np.float32)
    gx, gz = np.meshgrid(g, g, indexing="ij")
    pos = np.stack([gx, np.zeros_like(gx), gz], axis=-1).reshape(-1, 3).astype(np.float32)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    tri = np.stack([np.stack([a, c, b], 1), np.stack([a, d, c], 1)], axis=1).reshape(-1, 3).astype(np.uint32)
    col = rng.uniform(0.05, 0.95, (n * n, 3)).astype(np.float32)
    col = {"random": col, "zero": np.zeros_like(col), None: None}[colors]
    bsdf = {"lambertian": lambda: sd.lambertian(VERTEX_COLORS), "white": lambda: sd.lambertian(1.0), "black": lambda: sd.lambertian(0.0),
            "phong": lambda: sd.phong(12.0, rd=0.0, rs=VERTEX_COLORS, kd=0.5, ks=0.5),
            "phong_white": lambda: sd.phong(12.0, rd=0.0, rs=1.0, kd=0.5, ks=0.5)}[material]()
    sd.add_mesh(pos, tri, bsdf=bsdf, face_normals=True, name="grid", colors=col)
    sd.point_light((0.3, 1.5, -0.2), (5.0, 4.0, 3.0))
    sd.camera = dict(origin=(0.0, 2.0, 0.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), ortho_scale=1.0)
    sd.max_depth = 2
    return sd


def cornell_vcol(sky=False, sphere_subdiv=2):
    """C1's box with two coloured meshes inside: an icosphere with smooth normals whose Lambertian reflectance is its vertex
    colours (a function of the position), and a tilted grid whose twosided Phong takes them as specularReflectance; next to
    them an uncoloured mesh and, with sky = True, the sky luminaire as background (the front of the box is open)"""
    sd = cornell_c1()
    sd.name = "cornell_vcol_sky" if sky else "cornell_vcol"
    pos, tri = icosphere(sphere_subdiv, 0.35, (-0.35, 0.35, -0.2))
    col = (F(0.5) + F(0.45) * np.sin(pos * F(9.0) + np.array([0.0, 2.0, 4.0], dtype=np.float32))).astype(np.float32)
    sd.add_mesh(pos, tri, bsdf=sd.lambertian(VERTEX_COLORS), face_normals=False, name="coloured sphere", colors=col)
    g = vcol_grid(3, seed=11).meshes[0]
    c_, s_ = F(np.cos(0.6)), F(np.sin(0.6))
    p = g.positions * F(0.3)
    p = np.stack([p[:, 0], p[:, 2] * s_ + F(0.5), p[:, 2] * c_], axis=1) + np.array([0.45, 0.0, 0.25], dtype=np.float32)
    sd.add_mesh(p.astype(np.float32), g.triangles, bsdf=sd.twosided(sd.phong(20.0, rd=0.3, rs=VERTEX_COLORS, kd=0.6, ks=0.4)),
                face_normals=True, name="coloured sheet", colors=g.colors)
    pos, tri = icosphere(1, 0.2, (0.1, 0.2, 0.6))
    sd.add_mesh(pos, tri, bsdf=sd.roughmetal(0.2), face_normals=False, name="plain sphere")
    if sky:
        sd.sky(sun_direction=(0.3, 0.2, 0.8), turbidity=3.0, sky_scale=0.2)
    sd.max_depth = 5
    return sd


def tex_grid_mesh(cells=4, seed=3):
    """vcol_grid's planar grid (the same triangles in the same order) with per-triangle, unshared vertices -> (positions,
    triangles, texcoords).  The texcoords are a sheared affine map of (x, z) that reaches below zero, plus an offset of its
    own per triangle, so that uv jumps across every edge: a texcoord fetched from the neighbour's vertex shows"""
    g = vcol_grid(cells).meshes[0]
    pos = g.positions[g.triangles.ravel()].astype(np.float32)
    tri = np.arange(pos.shape[0], dtype=np.uint32).reshape(-1, 3)
    rng = np.random.RandomState(seed)
    M = np.array([[0.9, -0.35], [0.3, 0.8]], dtype=np.float32)
    uv = (pos[:, [0, 2]] @ M.T + np.array([-0.15, 0.1], dtype=np.float32)).astype(np.float32)
    uv = (uv.reshape(-1, 3, 2) + rng.uniform(-0.02, 0.02, (tri.shape[0], 1, 2)).astype(np.float32)).reshape(-1, 2)
    return pos, tri, uv.astype(np.float32)


def tex_scene(reflectance, shape="grid", cells=4, env=0.25, sky=False):
    """A Lambertian floor (shape = "grid": tex_grid_mesh in the plane y = 0) or one sphere (shape = "sphere") under a point
    light and a constant environment (or, sky = True, the sky), seen straight down by an orthographic camera, maxDepth 2.
    Neither shape can be hit twice by one path, so every radiance sample is linear in the reflectance at the camera hit.
    reflectance: a Checkerboard / GridTexture, a grey level or an RGB triple"""
    sd = SceneDescription("tex_%s" % shape)
    bsdf = sd.lambertian(reflectance)
    if shape == "grid":
        pos, tri, uv = tex_grid_mesh(cells)
        sd.add_mesh(pos, tri, bsdf=bsdf, face_normals=True, name="floor", texcoords=uv)
    else:
        sd.add_sphere((0.05, -0.1, -0.02), 0.8, bsdf=bsdf)
    sd.point_light((0.3, 1.5, -0.2), (5.0, 4.0, 3.0))
    if sky:
        sd.sky(sun_direction=(0.3, 0.2, 0.8), turbidity=3.0, sky_scale=0.2, to_world=[1, 0, 0, 0, 0, 1, 0, -1, 0])
    else:
        sd.add_lum(abi.LUM_CONSTANT, [env, env, env])
    sd.camera = dict(origin=(0.0, 2.0, 0.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), ortho_scale=1.0)
    sd.max_depth = 2
    return sd


def cornell_tex(sky=False):
    """C1's box with a checkerboard on a sphere shape, a sheet whose twosided Phong takes a grid texture as
    diffuseReflectance (slot 0) and the mesh's vertex colours as specularReflectance (slot 1), a mesh without texcoords
    under a checkerboard (uv = (0, 0) all over) and an untextured rough metal; with sky = True the sky as background"""
    sd = cornell_c1()
    sd.name = "cornell_tex_sky" if sky else "cornell_tex"
    check = Checkerboard(bright=(0.8, 0.7, 0.2), dark=(0.1, 0.15, 0.4), uscale=6.0, vscale=-3.0, uoffset=0.25)
    sd.add_sphere((-0.35, 0.35, -0.2), 0.35, bsdf=sd.lambertian(check))
    pos, tri, uv = tex_grid_mesh(3, seed=11)
    c_, s_ = F(np.cos(0.6)), F(np.sin(0.6))
    p = pos * F(0.3)
    p = np.stack([p[:, 0], p[:, 2] * s_ + F(0.5), p[:, 2] * c_], axis=1) + np.array([0.45, 0.0, 0.25], dtype=np.float32)
    col = (F(0.5) + F(0.45) * np.sin(pos * F(5.0) + np.array([0.0, 2.0, 4.0], dtype=np.float32))).astype(np.float32)
    grid = GridTexture(bright=(0.7, 0.7, 0.6), dark=0.05, uscale=3.7, vscale=-3.7, uoffset=0.3, voffset=-0.3, line_width=0.08)
    sd.add_mesh(p.astype(np.float32), tri, bsdf=sd.twosided(sd.phong(20.0, rd=grid, rs=VERTEX_COLORS, kd=0.6, ks=0.4)),
                face_normals=True, name="textured sheet", colors=col, texcoords=uv)
    pos, tri = icosphere(1, 0.2, (0.1, 0.2, 0.6))
    sd.add_mesh(pos, tri, bsdf=sd.microfacet(0.2, rd=check, rs=0.5), face_normals=False, name="no texcoords")
    pos, tri = icosphere(1, 0.15, (0.5, 0.15, -0.4))
    sd.add_mesh(pos, tri, bsdf=sd.roughmetal(0.2), face_normals=False, name="plain sphere")
    if sky:
        sd.sky(sun_direction=(0.3, 0.2, 0.8), turbidity=3.0, sky_scale=0.2)
    sd.max_depth = 5
    return sd


def cornell_bmp(sky=False, wrap="repeat"):
    """cornell_tex with an unfiltered 5 x 3 bitmap in place of the sphere's checkerboard: a bitmap, a checkerboard (the mesh
    without texcoords), a grid texture and vertex colours (the sheet's two slots) on different slots of one scene"""
    sd = cornell_tex(sky)
    sd.name = "cornell_bmp_sky" if sky else "cornell_bmp"
    texels = np.random.RandomState(9).uniform(0.05, 0.9, (3, 5, 3)).astype(np.float32)
    bmp = BitmapTexture(texels=texels, wrap=wrap, uscale=6.0, vscale=-3.0, uoffset=0.25)
    sd.meshes[[m.name for m in sd.meshes].index("sphere")].bsdf = sd.lambertian(bmp)
    return sd


def by_name(name, **kw):
    return {"c1": cornell_c1, "c3": cornell_c3, "c5": cornell_c5, "next": next_rows, "spheres": spheres, "envlit": envlit,
            "vcol_grid": vcol_grid, "vcol": cornell_vcol, "tex": cornell_tex, "bmp": cornell_bmp}[name](**kw)
