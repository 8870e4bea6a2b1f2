"""What the ctypes bindings of the nine shared objects have in common: where a library lies, how it is loaded and how a
return code becomes an exception.  Fails loudly: there is no CPU path."""
import ctypes as ct
import os

HERE = os.path.dirname(os.path.abspath(__file__))
MH_OK = 0
_vp, _u32, _u64, _int = ct.c_void_p, ct.c_uint32, ct.c_uint64, ct.c_int


class MuaHuffError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libmuahuff error %d: %s" % (code, msg))
        self.code = code


class Library:
    """One shared object of the product.  `module` is the binding's globals(): its SO and PROTOTYPES are read at the first
    lib(), not at import, so that a caller may point SO at another build before the first use."""

    def __init__(self, module, name, last_error):
        self.module, self.name, self.last_error, self.handle = module, name, last_error, None

    def lib(self):
        """Load the library.  Raises if it has not been built: the product has no fallback."""
        if self.handle is None:
            so = self.module["SO"]
            if not os.path.exists(so):
                raise ImportError(
                    "%s is missing (%s). Build it with `python __graft_entry__.py` or "
                    "`python hardware-efficient-mua-compression_amd/build.py`; there is no CPU fallback." % (self.name, so))
            # torch first: its wheel bundles the HIP runtime, and a process must not end up with two of them -- a
            # libmuahuff.so loaded before torch binds the system libamdhip64, torch then brings its own, and the
            # library's runtime finds no device (seen as MH_ERR_NO_DEVICE when build() and smoke() share a process)
            import torch  # noqa: F401
            l = ct.CDLL(so)
            for name, (res, args) in self.module["PROTOTYPES"].items():
                f = getattr(l, name)
                f.restype, f.argtypes = res, args
            self.handle = l
        return self.handle

    def check(self, rc):
        if rc != MH_OK:
            raise MuaHuffError(rc, getattr(self.lib(), self.last_error)().decode(errors="replace"))
        return rc
