from .g711 import g711_decode  # noqa: F401
